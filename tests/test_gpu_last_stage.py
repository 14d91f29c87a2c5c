"""-m gpu: the LAST stage of the saliency pass -- the per-frame maximum (k_smooth_down_mfma's reduction and atomicMax on encoded
floats) and k_quantise / k_quantise_profile -- checked per pixel against the interval that a correct fp32 evaluation of
u8 = trunc(255 expf(pre - max)) must land in (oracle/last_stage_ref.py: map_interval, derived from the roundings, not measured).

Every check reads PRE and the map from the SAME device run, so neither the network's fp32 noise nor a float64 convolution enters:
(a) directed logit fields through the doors SVC_NODE_MAP and SVC_NODE_MAP_PROFILE at every shape of test_net_plan_census.SHAPES;
(b) frame attribution at a full pass of the handle's chunk;
(c) the four saliency entries on real passes, each against its own TAP_PRE, including the maps whose h * w is 2^16 and more;
(d) the reference's formulation (oracle.unisal_ref.quantise_u8) on the device's PRE: where it differs from the device's map.

With SVC_LAST_STAGE_REPORT=<file> the counts of the run are written there as the table of profiles/last_stage.md."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import last_stage_cases as LS
import net_node_cases as C
from oracle import last_stage_ref as L, unisal_ref as U
from retargetvid_amd import ops, synth
from test_net_plan_census import SHAPES

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

DOOR_SHAPES = list(SHAPES) + [(140, 250)]               # the door plans like svc_saliency_u8: it accepts every shape of the table
CHUNK = int(os.environ.get('SVC_CHUNK') or 32)          # frames of one pass
_id = lambda s: '%dx%d' % s
_REPORT = []                                            # (section, case, stats) of this run


@pytest.fixture(scope='module')
def engines(synthetic_sd):
    """Handles by checkpoint ('carrier', 'ri', 'tl'), made on first use; the module's report is written when they close."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    made = {}

    def get(ck):
        if ck not in made:
            made[ck] = ops.Engine(synthetic_sd if ck == 'carrier' else C.checkpoint(ck)[0])
        return made[ck]
    yield get
    for e in made.values():
        e.close()
    path = os.environ.get('SVC_LAST_STAGE_REPORT')
    if path:
        with open(path, 'w') as f:
            f.write('| section | case | pixels | ambiguous | took lo | took hi | quantise_u8 differs |\n|---|---|---|---|---|---|---|\n')
            for section, case, s in _REPORT:
                f.write('| %s | %s | %d | %d | %d | %d | %s |\n' % (section, case, s['pixels'], s['ambiguous'], s['took_lo'], s['took_hi'],
                                                                 s.get('ref_differs', '-')))


def _door(eng, node, n, shape, logit):
    h, w = shape
    out = eng.run_node(C.DEV_NODE[node], n, h, w, logit, None, C.node_io(node, 0, 0, h, w)[2])
    assert out.shape == (n, 2, h, w)
    return out


def _both_doors(eng, n, shape, logit, where):
    """One run of each map node: the same bytes in both planes, nothing unwritten -> (PRE [n, h, w], map [n, h, w] as integers)."""
    a, b = _door(eng, 'map', n, shape, logit), _door(eng, 'map_profile', n, shape, logit)
    for name, out in (('map', a), ('map_profile', b)):
        assert not np.isnan(out[:, 0]).any(), (where, name, 'PRE left unwritten', int(np.isnan(out[:, 0]).sum()))
        assert not np.isnan(out[:, 1]).any(), (where, name, 'map bytes left unwritten', int(np.isnan(out[:, 1]).sum()),
                                               np.argwhere(np.isnan(out[:, 1]))[:4].tolist())
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (where, 'k_quantise and k_quantise_profile differ',
                                                                   np.argwhere(a != b)[:4].tolist())
    u = a[:, 1].astype(np.int64)
    assert np.array_equal(u, a[:, 1]) and u.min() >= 0 and u.max() <= 255, where
    return a[:, 0], u


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', DOOR_SHAPES, ids=_id)
def test_directed_fields_through_both_doors(engines, shape):
    """Three frames per call.  Every rule of map_interval at every pixel, from both kernels; plane 0 is SVC_NODE_SMOOTH's output."""
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    eng = engines('carrier')
    total = {}
    for name, logit in LS.fields(NH // 8, NW // 8).items():
        where = (shape, name)
        pre, u = _both_doors(eng, 3, shape, logit, where)
        smooth = eng.run_node(ops.NODE_SMOOTH, 3, h, w, logit, None, (h, w))
        assert np.array_equal(smooth.view(np.uint32), pre.view(np.uint32)), (where, 'plane 0 is not the smooth node\'s output')
        case = {}
        for i in range(3):
            case = LS.add(case, LS.check_frame(pre[i], u[i], where + (i,)))
            if name == 'flat':                                      # every pixel the maximum, up to the smoothing's own rounding
                assert np.ptp(pre[i]) <= 1e-4 * np.abs(pre[i]).max(), (where, i, 'the flat field is not flat on the device')
                assert (u[i][pre[i] == pre[i].max()] == 255).all() and u[i].min() >= 254, (where, i)
            if name == 'deep':                                      # zeros exactly where v* < 0.5
                v = 255.0 * np.exp(pre[i].astype(np.float64) - float(pre[i].max()))
                assert (u[i][v < 0.5] == 0).all() and (u[i][v >= 1.0 + 1e-6] > 0).all() and (v < 0.5).any(), (where, i)
            if name == 'apart':                                     # the frames' maxima are far apart, each map has its own 255
                assert u[i].max() == 255 and (u[i] < 255).any(), (where, i)
        if name != 'flat':
            LS.check_cap(case, where)
        else:
            print(where, 'spread of PRE in ulps', [float(np.ptp(pre[i]) / np.spacing(np.abs(pre[i]).max())) for i in range(3)],
                  'pixels below 255', int((u < 255).sum()))
        total = LS.add(total, case)
        if name == 'apart':
            m = pre.reshape(3, -1).max(1)
            assert m[0] - m[1] > 100 and m[1] - m[2] > 100, (where, m.tolist())
        if name == 'negative':
            assert pre.max() < 0, where
        if name == 'signed_zero':
            print(where, 'maxima', pre.reshape(3, -1).max(1).tolist(), 'negative zeros in PRE', int((np.signbit(pre) & (pre == 0)).sum()))
        if name == 'levels3':
            print(where, 'grey levels occupied', [len(np.unique(u[i])) for i in range(3)])
    _REPORT.append(('a: fields, both doors', _id(shape), total))


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(19, 250), (8, 8)], ids=_id)
def test_every_frame_of_a_full_pass_is_quantised_against_its_own_maximum(engines, shape):
    """n = the handle's chunk.  19x250: h * w is no multiple of 256, so frames share workgroups of k_quantise; 8x8: one workgroup
    holds four frames.  Offsets alternate +5000 and -5000, so a pixel quantised against a neighbouring frame's maximum is 0 where
    it should not be or 255 where it should not be."""
    NH, NW = U.get_optimal_out_size(shape)
    assert (shape[0] * shape[1]) % 256 != 0 or shape == (8, 8)
    logit = LS.attribution_logits(CHUNK, NH // 8, NW // 8)
    pre, u = _both_doors(engines('carrier'), CHUNK, shape, logit, shape)
    m = pre.reshape(CHUNK, -1).max(1)
    assert (m[0::2] > 1000).all() and (m[1::2] < -1000).all(), m.tolist()
    total = {}
    for i in range(CHUNK):
        total = LS.add(total, LS.check_frame(pre[i], u[i], (shape, i)))
        assert u[i].max() == 255, (shape, i)
    LS.check_cap(total, shape)
    _REPORT.append(('b: full pass of %d' % CHUNK, _id(shape), total))


# ---- (c), (d) -------------------------------------------------------------------------------------------------------------------
def _pass(eng, frames, where, **kw):
    """One saliency() call -> (its maps [n, h, w] as integers, its own TAP_PRE [n, h, w])."""
    n, h, w = frames.shape[:3]
    maps = eng.saliency(frames, **kw).cpu().numpy().astype(np.int64)
    pre = np.stack([eng.tap(ops.TAP_PRE, i, (h, w)) for i in range(n)])
    assert maps.shape == (n, h, w) and np.isfinite(pre).all(), where
    return maps, pre


def _check_pass(maps, pre, where, thr=0):
    total = {}
    for i in range(len(maps)):
        total = LS.add(total, LS.check_frame(pre[i], maps[i], where + (i,), thr=thr))
    LS.check_cap(total, where)
    return total


def _ref_differs(maps, pre, where):
    """(d) The reference's formulation, exp(log_softmax(x)) / max * 255 in fp32, on the device's PRE.  It rounds where the device
    does not: ls_x = fl(log_softmax(x)) and ls_max, each an absolute error 2^-24 |ls| that exp turns into a relative one; two
    exponentials at 1 ulp = 2^-23; the quotient and the product by 255 at 2^-24 each; 2^-23 of slack (last_stage_ref.ref_interval:
    delta_ref = 2^-24 (|ls_x| + |ls_max|) + 4 2^-23).  A pixel where the two maps differ must be ambiguous under delta_ref --
    the two sides then round one real number differently; anything else is an error of one of them.  -> the count."""
    ref = U.quantise_u8(torch.from_numpy(pre)).astype(np.int64)
    count = 0
    for i in range(len(maps)):
        diff = ref[i] != maps[i]
        lo, hi = L.ref_interval(pre[i])
        bad = diff & (lo == hi)
        assert not bad.any(), (where, i, 'quantise_u8 and the device differ at an unambiguous pixel', int(bad.sum()),
                               L.describe(pre[i], maps[i], bad), ref[i][bad][:4].tolist())
        assert (np.abs(ref[i] - maps[i]) <= 1).all(), (where, i)
        count += int(diff.sum())
    return count


@pytest.mark.parametrize('gname', ['16x9', 'port', '4x3'])
@pytest.mark.parametrize('ck', ['carrier', 'ri', 'tl'])
def test_the_four_entries_on_real_passes_against_their_own_pre(engines, ck, gname):
    """Goldens' frames at 140x250, 250x140 and 187x250: saliency() plain, threshold= 1, 120 and 255, census= and the profile entry
    (with and without a threshold), each output against the interval from that pass's own TAP_PRE; every entry gives the plain
    map's bytes behind its threshold; and (d) on the plain pass."""
    eng = engines(ck)
    frames = torch.from_numpy(C.golden_frames('ri' if ck == 'carrier' else ck, gname)).cuda()
    n, h, w = frames.shape[:3]
    assert (h, w) == {'16x9': (140, 250), 'port': (250, 140), '4x3': (187, 250)}[gname]
    where = (ck, gname)
    plain, pre = _pass(eng, frames, where)
    stats = _check_pass(plain, pre, where + ('plain',))
    stats['ref_differs'] = _ref_differs(plain, pre, where)
    _REPORT.append(('c, d: entries', '%s %s' % where, stats))
    cut = lambda t: np.where(plain < t, 0, plain)
    for t in (1, 120, 255):
        maps, p = _pass(eng, frames, where, threshold=t)
        _check_pass(maps, p, where + ('threshold', t), thr=t)
        assert np.array_equal(p.view(np.uint32), pre.view(np.uint32)) and np.array_equal(maps, cut(t)), where + ('threshold', t)
    rows = torch.zeros((n, 4), dtype=torch.int32, device='cuda')
    maps, p = _pass(eng, frames, where, threshold=120, census=rows)
    _check_pass(maps, p, where + ('census',), thr=120)
    assert np.array_equal(maps, cut(120)), where + ('census',)
    got = rows.cpu().numpy()[:, :3]
    assert np.array_equal(got, np.stack([(plain == v).reshape(n, -1).sum(1) for v in (119, 120, 121)], 1)), where + ('census rows',)
    for t in (0, 120):
        prof = torch.zeros((n, h + w), dtype=torch.int32, device='cuda')
        maps, p = _pass(eng, frames, where, threshold=t, profile=prof)
        _check_pass(maps, p, where + ('profile', t), thr=t)
        assert np.array_equal(maps, cut(t)), where + ('profile', t)
        assert np.array_equal(prof.cpu().numpy(), np.concatenate((plain.max(2), plain.max(1)), 1)), where + ('profile rows', t)


@pytest.mark.parametrize('shape', [(416, 256), (540, 960)], ids=_id)
def test_the_big_maps_whose_divisor_is_two_to_the_sixteen_and_more(engines, shape):
    """The maps the saliency entry takes and the tail does not, n = 3: k_quantise divides its index by h * w = 106 496 and 518 400."""
    h, w = shape
    assert h * w >= 1 << 16
    rng = np.random.RandomState(h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    fr = np.stack([rng.randint(0, 256, (h, w, 3)), np.stack([(xx * 255) // w, (yy * 255) // h, (xx + yy) % 256], 2),
                   synth.blob_frames(1, h, w, seed=h)[0]]).astype(np.uint8)
    frames = torch.from_numpy(fr).cuda()
    eng = engines('carrier')
    plain, pre = _pass(eng, frames, shape)
    stats = _check_pass(plain, pre, (shape, 'plain'))
    stats['ref_differs'] = _ref_differs(plain, pre, shape)
    _REPORT.append(('c, d: big maps', _id(shape), stats))
    maps, p = _pass(eng, frames, shape, threshold=120)
    _check_pass(maps, p, (shape, 'threshold'), thr=120)
    prof = torch.zeros((3, h + w), dtype=torch.int32, device='cuda')
    maps, p = _pass(eng, frames, shape, profile=prof)
    _check_pass(maps, p, (shape, 'profile'))
    assert np.array_equal(maps, plain), shape
