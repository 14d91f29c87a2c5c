"""The last stage without a GPU: the interval helper (oracle/last_stage_ref.py) on hand-made cases; the cap on ambiguous pixels for
the directed fields of tests/test_gpu_last_stage.py on the float64 smoothing oracle's PRE; and the reference's own fp32
formulation (oracle.unisal_ref.quantise_u8) inside the interval of its extra roundings on the goldens' maps."""
import functools
import os

import numpy as np
import pytest
import torch

import last_stage_cases as LS
from oracle import last_stage_ref as L, unisal_nodes_ref as N, unisal_ref as U
from retargetvid_amd import weights

f32 = np.float32


def test_a_tie_at_the_maximum_and_signed_zeros():
    pre = np.array([[1.5, -2.0, 1.5], [0.0, 1.0, -7.25]], f32)
    lo, hi, is_max = L.map_interval(pre)
    assert is_max.tolist() == [[True, False, True], [False, False, False]]
    assert lo[is_max].tolist() == [254, 254] and hi[is_max].tolist() == [255, 255]         # the formula; the exact rule decides there
    assert lo[1, 1] == hi[1, 1] == int(255 * np.exp(-0.5)) == 154
    u = np.array([[255, 7, 255], [56, 154, 0]])
    assert (lo[0, 1], lo[1, 0], lo[1, 2]) == (7, 56, 0) and np.array_equal(lo[~is_max], hi[~is_max])
    assert not L.violations(u, lo, hi, is_max).any()
    u[0, 2] = 254                                                                          # inside {lo, hi}, but a maximum
    assert L.violations(u, lo, hi, is_max).tolist() == [[False, False, True], [False, False, False]]
    # -0.0 against +0.0: equal, both are the maximum
    pre = np.array([[-0.0, 0.0], [-1.0, -0.0]], f32)
    lo, hi, is_max = L.map_interval(pre)
    assert is_max.tolist() == [[True, True], [False, True]] and lo[1, 0] == hi[1, 0] == 93


def test_far_below_the_maximum_and_an_all_negative_map():
    with np.errstate(all='raise'):                                  # no overflow, no invalid operation on the way
        pre = np.array([[3.0, 3.0 - 6.2, 3.0 - 6.3, 3.0 - 104.5, 3.0 - 1000.0, -3.0e38]], f32)
        lo, hi, is_max = L.map_interval(pre)
    assert lo.tolist() == [[254, 0, 0, 0, 0, 0]] and hi.tolist() == [[255, 0, 0, 0, 0, 0]] and is_max.tolist() == [[True] + [False] * 5]
    assert 255 * np.exp(-6.2) > 0.5 > 255 * np.exp(-6.3)            # v* = 0.517 truncates to 0 by floor, 0.468 by the rule
    # all negative: the interval depends on pre - m alone
    d = np.array([[0.0, -1.0], [-0.125, -5.5]], f32)
    for off in (0.0, -5000.0, -3.0e5):                             # (fp32 numbers all: an ulp at 3e5 is 2^-5)
        lo, hi, is_max = L.map_interval(d + f32(off))
        assert is_max.tolist() == [[True, False], [False, False]]
        assert lo[~is_max].tolist() == hi[~is_max].tolist() == [93, 225, 1]


def test_an_ambiguous_pixel_and_the_threshold_rule():
    # v* within delta of an integer: 255 exp(d) = 128 (1 + 1e-8)
    d = f32(np.log(128.0 / 255.0))
    pre = np.array([[0.0, d, np.nextafter(d, f32(-1)), np.nextafter(d, f32(0))]], f32)
    lo, hi, _ = L.map_interval(pre)
    v = 255 * np.exp(pre.astype(np.float64))
    assert abs(v[0, 1] / 128 - 1) < 2.0 ** -24 * abs(float(d)) + 2 * 2.0 ** -23
    assert (lo[0, 1], hi[0, 1]) == (127, 128)
    assert L.map_interval(pre, ulp_exp=8)[0][0, 2] == 127           # a wider documented bound widens the interval, nothing else does
    _, _, is_max = L.map_interval(pre)
    for t, ok, not_ok in ((0, (127, 128), (126, 129, 0)), (127, (127, 128), (0, 126)), (128, (0, 128), (127,)), (129, (0,), (127, 128)),
                          (255, (0,), (127, 128))):
        for val, want in [(a, False) for a in ok] + [(a, True) for a in not_ok]:
            u = np.array([[255, val, lo[0, 2] if lo[0, 2] >= t else 0, hi[0, 3] if hi[0, 3] >= t else 0]])
            assert L.violations(u, lo, hi, is_max, t)[0, 1] == want, (t, val)
            assert not L.violations(u, lo, hi, is_max, t)[0, [0, 2, 3]].any(), (t, val)
    u = np.array([[0, 0, 0, 0]])                                    # the maximum survives every threshold: 255 >= t
    assert L.violations(u, lo, hi, is_max, 255)[0, 0]


def test_the_reference_interval_contains_the_devices():
    rng = np.random.RandomState(3)
    pre = (3 * rng.standard_normal((40, 50))).astype(f32)
    lo, hi, _ = L.map_interval(pre)
    rlo, rhi = L.ref_interval(pre)
    assert (rlo <= lo).all() and (hi <= rhi).all()


# ---- the cap on the oracle's PRE ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _node_ref():
    sd = weights.make_synthetic_state_dict(0)
    return N.NodeRef(weights.fold_state_dict(sd), sd['smoothing_salicon.weight'], bounds=False)


@pytest.mark.parametrize('shape', [(140, 250), (8, 8), (250, 35)], ids=lambda s: '%dx%d' % s)
def test_the_directed_fields_keep_the_cap_on_the_oracles_pre(shape):
    """The float64 smoothing oracle's PRE, rounded to fp32, of every directed field: at most 1e-3 of a frame's pixels are ambiguous
    (the flat field: every pixel is the maximum).  A field that broke the cap would test nothing at those pixels."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    worst = 0.0
    for name, logit in LS.fields(NH // 8, NW // 8).items():
        pre = _node_ref().run('smooth', logit, out_hw=shape)[0].astype(f32)
        assert pre.shape == (3, h, w)
        case = {}
        for i in range(3):
            if name == 'flat':
                assert np.ptp(pre[i]) <= 4 * np.spacing(np.abs(pre[i]).max()), (shape, i, 'the flat field is not flat')
            # floor(v*) itself obeys the rules, as the map of an evaluation without rounding
            v = np.floor(255.0 * np.exp(pre[i].astype(np.float64) - pre[i].max())).astype(int)
            case = LS.add(case, LS.check_frame(pre[i], v, (shape, name, i)))
            if name == 'deep':
                assert (v == 0).mean() > 0.5
            if name == 'apart':
                assert abs(float(pre[i].max()) - (5000, 0, -5000)[i]) < 100
        if name != 'flat':
            LS.check_cap(case, (shape, name))
            worst = max(worst, case['ambiguous'] / case['pixels'])
    print(shape, 'largest ambiguous share %.2e' % worst)


# ---- the reference's formulation on the goldens ---------------------------------------------------------------------------------
@pytest.mark.parametrize('npz,ck', [('unisal_golden2.npz', 'ri'), ('unisal_golden2.npz', 'nc'), ('unisal_golden3.npz', 'tl')])
def test_the_references_quantisation_lies_inside_its_interval_on_the_goldens(golden_dir, npz, ck):
    """The goldens hold the reference model's log-softmax maps (fp32) and its uint8 maps.  A log-softmax map is a PRE -- the
    last stage is invariant under a shift -- so oracle.unisal_ref.quantise_u8 of it, and the reference model's own map, must lie
    in {lo, hi} of ref_interval (delta_ref: the reference's roundings, oracle/last_stage_ref.py)."""
    g = np.load(os.path.join(golden_dir, npz))
    tags = [k[5:] for k in g.files if k.startswith('logp_' + ck + '_')]
    assert len(tags) >= 6, tags
    differ = 0
    for tag in tags:
        pre = g['logp_' + tag].astype(f32)
        lo, hi = L.ref_interval(pre)
        q = U.quantise_u8(torch.from_numpy(pre)[None])[0].astype(int)
        for what, u in (('quantise_u8', q), ('the reference model', g['u8_' + tag].astype(int))):
            bad = (u != lo) & (u != hi)
            assert not bad.any(), (tag, what, int(bad.sum()), L.describe(pre, u, bad))
        dlo, dhi, _ = L.map_interval(pre)
        differ += int(((q != dlo) & (q != dhi)).sum())
    print(ck, 'pixels of quantise_u8 outside the DEVICE interval of the same PRE:', differ)
