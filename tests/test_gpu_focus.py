"""-m gpu: the focus stability from maps that stay on the device -- svc_focus_jumps_u8 / k_focus_jumps behind ops.focus_jumps,
temporal.focus_stability_device, and after_ingest's route switch SVC_FOCUS.

The oracle is oracle/temporal_ref.mean_saliency_on_jump, row by row: a count of 0 goes with the oracle's 255 ("no statistic"),
otherwise sum / count EQUALS the oracle's mean -- the same integer sum divided by the same count in float64, not a close value.
tests/focus_cases.py builds the random battery (as tests/test_host_native.py builds its own) and its census; the directed rows
below are what the battery lacks.  Every launch is a few dozen wavefronts."""
import functools

import numpy as np
import pytest
import torch

import focus_cases as F
import refpath_cases as RC
from oracle import pipeline_ref as P, temporal_ref as TR
from poison import FILL, poisoned_outputs  # noqa: F401  (fixture)
from retargetvid_amd import ops, smartVidCrop as S, temporal

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs')]

FILL_WORD = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])


@functools.lru_cache(maxsize=1)
def battery():
    return F.battery()


def run(maps, xy, min_d):
    """One launch -> int [n, 2] on the host; every word was written (none is the poison's fill)."""
    dev = maps if torch.is_tensor(maps) else torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    out = ops.focus_jumps(dev, xy, min_d)
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(xy), 2) and out.device == dev.device
    got = out.cpu().numpy()
    assert not (got == FILL_WORD).any()
    return got


def check_rows(got, maps, xy, min_d, what):
    """Rows against the oracle: row 0 = (0, 0); count 0 <=> the oracle's integer 255, and then sum 0; else sum / count == the mean."""
    ref = F.oracle_jumps(maps, np.asarray(xy, np.float64), min_d)
    assert got[0].tolist() == [0, 0], what
    for i in range(1, len(ref)):
        s, c = int(got[i, 0]), int(got[i, 1])
        assert c >= 0 and (c == 0) == (type(ref[i]) is int), (what, i, s, c, ref[i])
        assert (s / c if c else 255) == ref[i] and (c or s == 0), (what, i, s, c, ref[i])
    return ref


def test_battery_every_row_equals_the_oracle_and_no_class_of_rows_is_empty():
    """48 trials x min_d 1 and 10 = 2 054 rows, one launch per trial and min_d.  The census from the oracle (1 585 rows with a
    statistic, 469 below min_d; 864 with more than 64 samples -- a lane takes more than one --, 340 with more than 128, 18 with
    exactly 64 and 12 with 65; 583 along one axis; 76 clipped at the image edge) is recomputed and every class must be
    non-empty, so that a changed generator cannot empty one silently."""
    cases = battery()
    census = F.census(cases)
    print(census)
    assert census['rows'] == sum(len(xy) - 1 for _, _, xy in cases) * len(F.MIN_DS) > 2000
    assert all(v > 0 for v in census.values()), census
    assert census['statistic'] + census['below_min_d'] <= census['rows'] and census['m_gt_128'] < census['m_gt_64']
    n_stats = 0
    for trial, maps, xy in cases:
        dev = torch.from_numpy(maps).cuda()
        for min_d in F.MIN_DS:
            ref = check_rows(run(dev, xy, min_d), maps, xy, min_d, (trial, min_d))
            n_stats += sum(type(v) is not int for v in ref)
    assert n_stats == census['statistic']


SEVENS = np.full((2, 35, 62), 7, np.uint8)


@pytest.mark.parametrize('p1, p2, want', [
    ((5.1, 22.3), (15.1, 22.3), 255), ((11.7, 33.3), (31.7, 33.3), 255), ((50.4, 30.6), (63.4, 30.6), 255),     # NumPy's length mismatch
    ((10, 10), (11, 10), 7.0), ((10, 10), (11, 11), 7.0),                                                      # m == 1
    ((-3, -2), (-1, -1.5), 255), ((70, 3), (64, 5), 255),                                                      # both centres outside
    ((65000, 3), (-65000, 9), 7.0),                                                                            # the domain's far end
])
def test_directed_rows_on_a_map_of_sevens(p1, p2, want):
    xy = np.array([p1, p2], np.float64)
    ref = TR.mean_saliency_on_jump(SEVENS[1], float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1]), 1)
    assert ref == want and (type(ref) is int) == (want == 255)                  # the oracle says what the issue recorded
    got = run(SEVENS, xy, 1)
    check_rows(got, SEVENS, xy, 1, (p1, p2))
    if want == 255:
        assert got[1].tolist() == [0, 0]
    else:
        assert got[1, 1] > 0 and got[1, 0] == 7 * got[1, 1]


@pytest.mark.parametrize('p1, p2', [((1e5, 3), (-1e5, 9)), ((65536.5, 3), (10, 9)), ((float('nan'), 3), (10, 9)), ((10, 3), (10, float('inf'))),
                                    ((10, float('-inf')), (10, 9)), ((10, 3), (float('nan'), float('nan')))])
def test_a_move_outside_the_domain_is_row_0_minus_1_and_the_device_route_raises(p1, p2):
    """Not finite or beyond SVC_FOCUS_MAX_COORD: ops.focus_jumps returns { 0, -1 } for the move (the moves around it are computed),
    temporal.focus_stability_device raises ValueError naming it."""
    xy = np.array([(3, 4), (20, 9), p1, p2, (30, 30)], np.float64)
    maps = np.full((5, 35, 62), 7, np.uint8)
    got = run(maps, xy, 1)
    assert got[3].tolist() == [0, -1]
    assert got[0].tolist() == [0, 0] and got[1, 1] > 0 and got[1, 0] == 7 * got[1, 1]
    bad = [i for i in range(1, 5) if not (np.abs(xy[i - 1:i + 1]) <= 65536).all()]
    assert [i for i in range(5) if got[i, 1] < 0] == bad and 3 in bad
    with pytest.raises(ValueError, match='move %d -> %d' % (bad[0] - 1, bad[0])):
        temporal.focus_stability_device(xy, torch.from_numpy(maps).cuda(), 30.0, P.init_crop_params(True))


def test_no_map_one_map_and_a_map_tensor_at_an_odd_address():
    empty = torch.zeros((0, 35, 62), dtype=torch.uint8, device='cuda')
    assert run(empty, np.zeros((0, 2)), 1).shape == (0, 2)
    CP = P.init_crop_params(True)
    xy, jumps, inds = temporal.focus_stability_device(np.zeros((0, 2)), empty, 30.0, CP)
    assert xy.shape == (0, 2) and jumps == [] and inds == []
    assert run(SEVENS[:1], np.array([[3.0, 4.0]]), 1).tolist() == [[0, 0]]
    xy, jumps, inds = temporal.focus_stability_device(np.array([[3.0, 4.0]]), torch.from_numpy(SEVENS[:1]).cuda(), 30.0, CP)
    assert xy.tolist() == [[3.0, 4.0]] and jumps == [255] and inds == []
    trial, maps, cxy = battery()[4]                                     # 140 x 250, centres anywhere: long lines, some clipped
    big = torch.zeros(maps.size + 16, dtype=torch.uint8, device='cuda')
    for off in (1, 3):
        odd = big[off:off + maps.size].view(maps.shape)
        odd.copy_(torch.from_numpy(maps))
        assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
        check_rows(run(odd, cxy, 1), maps, cxy, 1, ('odd', off))
    with pytest.raises(TypeError):
        ops.focus_jumps(torch.from_numpy(maps).cuda()[:, :, ::2], cxy, 1)              # not contiguous
    with pytest.raises(ValueError):
        ops.focus_jumps(torch.from_numpy(maps).cuda(), cxy[:-1], 1)                    # one centre short


def test_device_route_equals_the_host_route_triple_for_triple():
    """focus_stability_device on the resident maps against focus_stability_native on their host copy: held centres, jump list (the
    integer 255 where there is no statistic, floats elsewhere) and index list, on six trials -- every shape and kind -- with
    foces_stab_t in (60, 120, 200) and both parameter sets."""
    n_inds = 0
    for k, t in enumerate((0, 5, 10, 15, 17, 22)):
        trial, maps, xy = battery()[t]
        dev = torch.from_numpy(maps).cuda()
        for stab_t in (60, 120, 200):
            CP = dict(P.init_crop_params(k % 2 == 0), foces_stab_t=stab_t)
            want = temporal.focus_stability_native(xy, dev.cpu().numpy(), 30.0, CP)
            got = temporal.focus_stability_device(xy, dev, 30.0, CP)
            assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype, (trial, stab_t)
            assert got[1] == want[1] and [type(v) for v in got[1]] == [type(v) for v in want[1]], (trial, stab_t)
            assert got[2] == want[2] and all(type(v) is int for v in got[2]), (trial, stab_t)
            n_inds += len(got[2])
    assert n_inds > 30


# ---- after_ingest ---------------------------------------------------------------------------------------------------------
class ResidentMaps(torch.Tensor):
    """Maps that refuse to leave the device: .cpu() of the [n, h, w] tensor raises (small results derived from it still travel)."""

    def cpu(self, *a, **k):
        if self.dim() == 3:
            raise AssertionError('the maps were copied to the host')
        return super().cpu(*a, **k)


class HostRouteReached(Exception):
    pass


def _case():
    cases, _ = RC.load()
    c = next(c for c in cases if RC.case_id(c) == '05_best_cuts_skip_plus_1')
    CP = S.sc_init_crop_params(use_best_settings=c['best'])
    CP.update(c['overrides'])
    assert CP['focus_stability'] and not CP['com_km'] and len(c['jumps_inds']) >= 2 and (c['jumps'] != 255).sum() >= 10
    return c, CP


def _vd(c, maps):
    return dict(smaps_dev=maps, segmentation=c['segmentation'].copy(), segmentation_sel=c['segmentation_sel'].copy(),
                true_inds=c['true_inds'].tolist(), inds_to_orig=c['inds_to_orig'].tolist(), fr=c['fr'], fc=c['fc'], fc_sel=c['fc_sel'],
                h_orig=c['h_orig'], w_orig=c['w_orig'], h_process=c['h_process'], w_process=c['w_process'],
                n_net_maps=int(c['raw'].reshape(c['fc_sel'], -1).any(1).sum()))


def _host_route_raises(*a, **k):
    raise HostRouteReached()


def test_after_ingest_takes_the_device_route_and_moves_no_map(engine, monkeypatch):
    """A best-settings video of tests/golden/refpath_golden.npz with the host route booby-trapped: focus_stability_native raises and
    the maps' .cpu() raises.  after_ingest finishes, and the jump statistics, their index list and the held centres are the
    reference's own (the fixture's), exactly."""
    c, CP = _case()
    monkeypatch.delenv('SVC_FOCUS', raising=False)
    monkeypatch.setattr(temporal, 'focus_stability_native', _host_route_raises)
    maps = torch.from_numpy(c['raw']).cuda().as_subclass(ResidentMaps)
    with pytest.raises(AssertionError, match='copied to the host'):
        maps.cpu()
    VD, res = S.after_ingest(_vd(c, maps), CP, engine)
    assert res['result'] == 'smart cropped' and 't__focus_stability' in res
    assert VD['jumps_inds'] == c['jumps_inds']
    assert [float(v) for v in VD['jumps']] == c['jumps'].tolist()
    assert np.array_equal(np.stack([VD['dx'], VD['dy']], 1), c['centres_stab'])
    assert not np.array_equal(c['centres_stab'], c['centres_filled'])                  # (the hold moved a centre in this video)
    monkeypatch.setenv('SVC_FOCUS', 'device')                                          # the default, spelled out
    VD2, _ = S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda().as_subclass(ResidentMaps)), CP, engine)
    assert VD2['jumps'] == VD['jumps'] and VD2['jumps_inds'] == VD['jumps_inds'] and VD2['dx'] == VD['dx'] and VD2['dy'] == VD['dy']


def test_after_ingest_route_switch(engine, monkeypatch):
    """SVC_FOCUS=host reaches focus_stability_native (and, unpatched, gives the fixture's values); an unknown spelling is a
    ValueError; with focus_stability off the variable is not read at all."""
    c, CP = _case()
    monkeypatch.setenv('SVC_FOCUS', 'host')
    VD, _ = S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda()), CP, engine)
    assert VD['jumps_inds'] == c['jumps_inds'] and [float(v) for v in VD['jumps']] == c['jumps'].tolist()
    assert np.array_equal(np.stack([VD['dx'], VD['dy']], 1), c['centres_stab'])
    with monkeypatch.context() as m:
        m.setattr(temporal, 'focus_stability_native', _host_route_raises)
        with pytest.raises(HostRouteReached):
            S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda()), CP, engine)
    monkeypatch.setenv('SVC_FOCUS', 'Device')
    with pytest.raises(ValueError, match='SVC_FOCUS'):
        S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda()), CP, engine)
    VD, _ = S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda()), dict(CP, focus_stability=False), engine)
    assert VD['jumps_inds'] == [] and VD['jumps'] == [255] * c['fc_sel']
