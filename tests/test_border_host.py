"""Border detection without a GPU: the host half of sc_border_detection (counting, the 45 % cap, the scaling to the original
frame) and the border arithmetic of the boxes against tests/golden/border_golden.npz -- the reference's OWN sc_border_detection
(smartVidCrop.py:842-924) and sc_compute_bb (:979-1048) run on seeded map stacks by tools/make_golden_border.py.  The device
half (the profile of the raw maps) is tests/test_gpu_border.py."""
import os

import numpy as np
import pytest

from oracle import tail_ref as T
from retargetvid_amd import scheduler, smartVidCrop as S, temporal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('border_t', 'border_b', 'border_l', 'border_r')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'border_golden.npz'))


def _case(z, i):
    h, w, ho, wo, tb, off = (int(v) for v in z['meta'][i])
    return h, w, ho, wo, tb, z['profiles'][off:off + h + w]


def test_fixture_covers_what_it_must(golden):
    z = golden
    assert len(z['meta']) >= 200 and len(set(z['box_case'].tolist())) >= 50
    kinds = set(z['kind'].tolist())
    assert {'nothing_above', 't0', 't254', 't255', 'single_pixel', 'top_only', 'bottom_only', 'left_only', 'right_only'} <= kinds
    sizes = {tuple(int(v) for v in m[:2]) for m in z['meta']}
    assert {(140, 250), (250, 140), (166, 250), (141, 250)} <= sizes
    assert {0, 254, 255} <= set(z['meta'][:, 4].tolist())
    for i in np.flatnonzero(z['kind'] == 'nothing_above'):             # all four hit the 0.45 cap
        h, w, ho, wo = (int(v) for v in z['meta'][i][:4])
        assert z['borders'][i].tolist() == [int((ho / h) * int(h * 0.45))] * 2 + [int((wo / w) * int(w * 0.45))] * 2
    assert set(z['box_ratio'].tolist()) == {'1:3', '3:1', '9:16'}


def test_border_detection_reproduces_every_reference_border(golden):
    z = golden
    for i in range(len(z['meta'])):
        h, w, ho, wo, tb, prof = _case(z, i)
        CP = S.sc_init_crop_params()
        CP['t_border'] = tb
        VD = dict(h_process=h, w_process=w, h_orig=ho, w_orig=wo, border_profile=prof.astype(np.int32))
        out = S.sc_border_detection(CP, VD)
        assert out is VD
        assert [VD[k] for k in KEYS] == z['borders'][i].tolist(), (i, str(z['kind'][i]))
        assert all(type(VD[k]) is int for k in KEYS)
        assert VD['border_f_col'].dtype == np.uint8 and np.array_equal(VD['border_f_col'], prof[:h])
        assert VD['border_f_row'].dtype == np.uint8 and np.array_equal(VD['border_f_row'], prof[h:])


def test_boxes_under_borders_equal_the_reference_and_the_oracle(golden):
    z = golden
    unfit = 0
    for k, c in enumerate(z['box_case']):
        h, w, ho, wo, tb, prof = _case(z, int(c))
        ratio = str(z['box_ratio'][k])
        CP = dict(S.sc_init_crop_params(), t_border=tb, out_ratio=ratio)
        VD = dict(h_process=h, w_process=w, h_orig=ho, w_orig=wo, border_profile=prof, fc=z['box_xy'].shape[1])
        S.sc_border_detection(CP, VD)
        brd = tuple(VD[key] for key in KEYS)
        assert any(brd)
        S.sc_calc_dest_size(VD, CP)
        xs, ys = z['box_xy'][k][:, 0], z['box_xy'][k][:, 1]
        bb, ctr, fw, fh = temporal.boxes(xs, ys, wo, ho, w, h, VD['w_final'], VD['h_final'], borders=brd)
        assert (fw, fh) == tuple(z['fbb'][k].tolist()), (k, ratio)
        assert np.array_equal(bb, z['boxes'][k]), (k, ratio)
        obb, ofw, ofh = T.compute_bb(xs.tolist(), ys.tolist(), len(xs), wo, ho, w, h, VD['w_final'], VD['h_final'], borders=brd)
        assert (ofw, ofh) == (fw, fh) and np.array_equal(np.asarray(obb), bb)
        # the whole path the package takes: sc_compute_bb on the dict
        VD['dxs'], VD['dys'] = xs.tolist(), ys.tolist()
        S.sc_compute_bb(VD, CP)
        assert np.array_equal(np.asarray(VD['bbs']), z['boxes'][k]) and (VD['fbb_w'], VD['fbb_h']) == (fw, fh)
        # size and position.  The reference shrinks the window only on the axis it spans fully; on the other axis a window can be
        # wider than what the borders leave (both bars at the 45 % cap: a tenth of the side), and then its own clamps cannot both
        # hold.  Every window that fits lies inside; the few that cannot are the reference's, reproduced above.
        t, b, l, r = brd
        assert ((bb[:, 2] - bb[:, 0]) == fw).all() and ((bb[:, 3] - bb[:, 1]) == fh).all()
        if fw <= wo - l - r and fh <= ho - t - b:
            assert (bb[:, 0] >= l).all() and (bb[:, 2] <= wo - r).all() and (bb[:, 1] >= t).all() and (bb[:, 3] <= ho - b).all()
        else:
            unfit += 1
    assert unfit <= 3           # (3 of the 167 records: cases 39, 81 and 171 of the generator)


def test_border_off_gives_four_zeros_and_touches_nothing_else():
    CP = S.sc_init_crop_params()
    assert CP['t_border'] == -1
    VD = dict(h_process=140, w_process=250, h_orig=360, w_orig=640, marker=object())
    before = dict(VD)
    out = S.sc_border_detection(CP, VD)
    assert out is VD and [VD[k] for k in KEYS] == [0, 0, 0, 0]
    assert {k: v for k, v in VD.items() if k not in KEYS} == before


def test_profile_of_the_wrong_length_and_missing_maps_are_errors():
    CP = dict(S.sc_init_crop_params(), t_border=10)
    with pytest.raises(ValueError):
        S.sc_border_detection(CP, dict(h_process=140, w_process=250, h_orig=360, w_orig=640, border_profile=np.zeros(389, np.int32)))
    with pytest.raises(ValueError):          # thresholded maps (the ingest ran the tail) and no profile: nothing to measure
        S.sc_border_detection(CP, dict(h_process=140, w_process=250, h_orig=360, w_orig=640, xy_stream=np.zeros((1, 2)), smaps_dev=None))
    with pytest.raises(ValueError):
        S.sc_border_detection(CP, dict(h_process=140, w_process=250, h_orig=360, w_orig=640))


def test_the_two_gates_still_raise_and_border_detection_no_longer_does():
    video = dict(fr=25.0, frame_count=0, w=640, h=360, frames=None, trans_inds=[])
    for key in ('exit_on_spread_sal', 'exit_on_low_cvrg'):
        CP = dict(S.sc_init_crop_params(), **{key: True})
        with pytest.raises(NotImplementedError) as e:
            S.smart_vid_crop(video, CP, save_vid=False, engine=object())
        assert 'exit_on_spread_sal' in str(e.value) and 'exit_on_low_cvrg' in str(e.value) and 'border' not in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            scheduler.JobScheduler(CP, engines=[])
        assert 'border' not in str(e.value)
    # t_border alone passes the refusal: the call gets as far as the next one (no reader installed for a file name)
    assert S._video_reader is None
    with pytest.raises(NotImplementedError) as e:
        S.smart_vid_crop('film.mp4', dict(S.sc_init_crop_params(), t_border=10), save_vid=False, engine=object())
    assert 'decoding video files' in str(e.value)
