"""Pins oracle/unisal_ref.py and oracle/lanczos_ref.py to outputs of the REFERENCE model code
(tests/golden/unisal_golden.npz, made by tools/make_golden_unisal.py) and of Pillow."""
import os

import pytest

import numpy as np
import torch

from oracle import lanczos_ref, unisal_ref as U


def test_optimal_out_size():
    assert U.get_optimal_out_size((140, 250)) == (256, 416)      # 16:9 -> (8,13)*32, SURVEY fact 3
    assert U.get_optimal_out_size((360, 640)) == (256, 416)
    assert U.get_optimal_out_size((250, 250)) == (320, 320)
    assert U.get_optimal_out_size((250, 140)) == (416, 256)


def test_lanczos_matches_pillow_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'lanczos_golden.npz'))
    for i in range(4):
        a, ref = g['in_%d' % i], g['out_%d' % i]
        got = lanczos_ref.resize_lanczos_u8(a, ref.shape[0], ref.shape[1])
        assert np.array_equal(got, ref), 'case %d differs from Pillow %s' % (i, g['pillow_version'])


def test_lanczos_matches_installed_pillow():
    PIL = __import__('pytest').importorskip('PIL.Image')
    a = np.random.RandomState(1).randint(0, 256, (140, 250, 3)).astype(np.uint8)
    ref = np.asarray(PIL.fromarray(a).resize((416, 256), PIL.LANCZOS))
    assert np.array_equal(lanczos_ref.resize_lanczos_u8(a, 256, 416), ref)


def test_forward_matches_reference_model(golden_dir, synthetic_sd):
    torch.set_num_threads(1)             # the golden was generated single-threaded
    g = np.load(os.path.join(golden_dir, 'unisal_golden.npz'))
    frames = g['frames']
    taps = {}
    maps = U.saliency_u8(synthetic_sd, frames, taps)
    assert maps.shape == (140, 250, frames.shape[0]) and maps.dtype == np.uint8
    t0 = taps['frames'][0]
    assert np.array_equal(t0['input'][0].numpy(), g['input_0'])
    for k in ('feat_1x', 'feat_2x', 'feat_4x', 'post_cnn'):
        ref = g[k + '_0']
        assert np.abs(t0[k][0].numpy() - ref).max() <= 1e-4 * np.abs(ref).max(), k
    d = np.abs(maps.astype(int) - g['smaps_u8'].astype(int))
    # same torch ops as the reference: identical up to thread-count dependent summation order
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    for i in range(frames.shape[0]):
        lp = torch.log_softmax(taps['frames'][i]['pre'].reshape(1, -1), 1).reshape(140, 250).numpy()
        assert np.abs(lp - g['logp_%d' % i]).max() < 1e-4


def _golden2_checkpoint(g, ck):
    from retargetvid_amd import weights
    if ck == 'nc':
        return weights.make_synthetic_state_dict(3, carrier=False)
    stats = {k[3:]: g[k] for k in g.files if k.startswith('bn/')}
    return weights.make_reference_init_state_dict(7, stats)


def test_forward_matches_reference_model_without_carrier_all_geometries(golden_dir):
    """tests/golden/unisal_golden2.npz (tools/make_golden_unisal2.py): the reference model on a non-carrier random
    checkpoint and on a reference-initialised one (BatchNorm statistics calibrated by the reference model itself),
    at the 16:9, 4:3 and portrait network geometries, every frame: log-softmax maps, u8 maps, taps of frame 0."""
    torch.set_num_threads(4)
    g = np.load(os.path.join(golden_dir, 'unisal_golden2.npz'))
    for ck in ('nc', 'ri'):
        sd = _golden2_checkpoint(g, ck)
        for gname in ('16x9', '4x3', 'port'):
            frames = g['frames_' + gname]
            h, w = frames.shape[1:3]
            taps = {}
            maps = U.saliency_u8(sd, frames, taps)
            for i in range(frames.shape[0]):
                tag = '%s_%s_%d' % (ck, gname, i)
                t = taps['frames'][i]
                lp = torch.log_softmax(t['pre'].reshape(1, -1), 1).reshape(h, w).numpy()
                assert np.abs(lp - g['logp_' + tag]).max() < 2e-5, tag
                d = np.abs(maps[:, :, i].astype(int) - g['u8_' + tag].astype(int))
                assert d.max() <= 1 and (d > 0).mean() < 2e-3, tag
                if i == 0:
                    for k in ('feat_2x', 'post_cnn'):
                        ref = g['%s_%s' % (k, tag)]
                        assert np.allclose(t[k][0].numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max()), (k, tag)
                    ref = g['adapt_' + tag]
                    assert np.allclose(t['adapt'][0].numpy(), ref[0], rtol=1e-4, atol=1e-5 * np.abs(ref).max()), tag
    # the reference-initialised maps are not flat: the u8 map spans well over 100 grey levels
    assert np.ptp(g['u8_ri_16x9_0']) > 100


@pytest.mark.parametrize('variant', [1, 2])
def test_forward_matches_reference_model_on_the_trained_like_checkpoint(golden_dir, variant):
    """tests/golden/unisal_golden3.npz (tools/make_golden_unisal3.py): the reference model with its last decoder stage FITTED
    to blob targets -- peaky maps like a trained network's -- at the three geometries, every frame."""
    from retargetvid_amd import weights
    torch.set_num_threads(4)
    g = np.load(os.path.join(golden_dir, 'unisal_golden3.npz' if variant == 1 else 'unisal_golden4.npz'))
    sd = weights.make_trained_like_state_dict(golden_dir, variant=variant)
    for gname in ('16x9', '4x3', 'port'):
        frames = g['frames_' + gname]
        h, w = frames.shape[1:3]
        taps = {}
        maps = U.saliency_u8(sd, frames, taps)
        for i in range(frames.shape[0]):
            tag = '%s_%s_%d' % ('tl' if variant == 1 else 'tl2', gname, i)
            t = taps['frames'][i]
            lp = torch.log_softmax(t['pre'].reshape(1, -1), 1).reshape(h, w).numpy()
            assert np.abs(lp - g['logp_' + tag]).max() < 1e-4, tag               # the log-softmax spans ~40 here (a peaky map)
            d = np.abs(maps[:, :, i].astype(int) - g['u8_' + tag].astype(int))
            assert d.max() <= 1 and (d > 0).mean() < 2e-3, tag
            if i == 0:
                ref = g['adapt_' + tag]
                assert np.allclose(t['adapt'][0].numpy(), ref[0], rtol=1e-4, atol=1e-5 * np.abs(ref).max()), tag
    # peaky: a few hundred points above the default threshold, a handful of pixels per grey level next to it
    hist = g['level_hist_16x9'] / 24.0
    assert 100 < hist[120:].sum() < 3000 and hist[110:131].mean() < 20


def test_quantise_is_floor_of_scaled_softmax():
    x = torch.randn(2, 140, 250)
    q = U.quantise_u8(x)
    m = x.reshape(2, -1).max(1).values.reshape(2, 1, 1)
    approx = np.floor(255.0 * torch.exp(x - m).double().numpy())
    assert np.abs(q.astype(int) - approx).max() <= 1
    assert q.max() == 255


# the eleven network input sizes get_optimal_out_size can select for saliency maps of at most 250 px, one map shape each
ELEVEN = {'16x9': (140, 250), '4x3': (187, 250), 'port': (250, 140), '3x2': (166, 250), '5x4': (200, 250), '11x10': (230, 250),
          '1x1': (249, 249), '10x11': (250, 230), '4x5': (250, 200), '3x4': (250, 187), '2x3': (250, 166)}
NET_SIZES = {'16x9': (256, 416), '4x3': (288, 384), 'port': (416, 256), '3x2': (288, 416), '5x4': (320, 384), '11x10': (320, 352),
             '1x1': (320, 320), '10x11': (352, 320), '4x5': (384, 320), '3x4': (384, 288), '2x3': (416, 288)}


def test_eleven_network_sizes_are_all_the_selectable_ones():
    """Every map of 8..250 x 250 and 250 x 8..250 selects one of the eleven sizes, and each of them is selected by its map shape."""
    got = {U.get_optimal_out_size((h, 250)) for h in range(8, 251)} | {U.get_optimal_out_size((250, w)) for w in range(8, 251)}
    assert got == set(NET_SIZES.values())
    for g, shape in ELEVEN.items():
        assert U.get_optimal_out_size(shape) == NET_SIZES[g], g


def golden5_frames(g, gname):
    """The frames of tests/golden/unisal_golden5.npz, regenerated from their seeds and checked against the stored SHA-256."""
    import hashlib
    from retargetvid_amd import synth
    from tools.make_golden_unisal5 import GEOMS, N, SEED
    h, w = GEOMS[gname]
    fr = synth.blob_frames(N, h, w, seed=SEED[gname])
    assert hashlib.sha256(fr.tobytes()).hexdigest() == str(g['frames_sha256_' + gname]), gname
    return fr


def golden5_u8(g, ck, gname, i):
    """(reference u8 map of frame i, index of the map's pixels it holds): the whole map for tl / tl2, every other row and column for
    nc / ri."""
    from tools.make_golden_unisal5 import FULL_U8, GEOMS, U8_STEP, decode_u8, grid
    h, w = GEOMS[gname]
    ref = decode_u8(g['u8_%s_%s_%d' % (ck, gname, i)])
    idx = np.ix_(np.arange(h), np.arange(w)) if ck in FULL_U8 else np.ix_(*grid(h, w, U8_STEP))
    assert ref.shape == (len(idx[0]), idx[1].shape[1]), (ck, gname, i)
    return ref, idx


def golden5_checkpoint(ck, golden_dir):
    from retargetvid_amd import weights
    if ck == 'nc':
        return weights.make_synthetic_state_dict(3, carrier=False)
    if ck == 'ri':
        g2 = np.load(os.path.join(golden_dir, 'unisal_golden2.npz'))
        return weights.make_reference_init_state_dict(7, {k[3:]: g2[k] for k in g2.files if k.startswith('bn/')})
    return weights.make_trained_like_state_dict(golden_dir, variant=1 if ck == 'tl' else 2)


@pytest.mark.parametrize('ck', ['nc', 'ri', 'tl', 'tl2'])
def test_forward_matches_reference_model_at_the_eight_other_geometries(golden_dir, ck):
    """tests/golden/unisal_golden5.npz (tools/make_golden_unisal5.py): the reference model at the eight network input sizes golden2-4
    do not reach (288x416, 320x384, 320x352, 320x320, 352x320, 384x320, 384x288, 416x288), every frame: u8 maps, and for frame 0 the
    adaptation output and the log-softmax map, at the gates of the three-geometry tests above -- on the pixels the golden holds
    (tools/make_golden_unisal5.py: grid samples, whole u8 maps for tl / tl2)."""
    from tools.make_golden_unisal5 import GEOMS, NET, grid
    torch.set_num_threads(4)
    g = np.load(os.path.join(golden_dir, 'unisal_golden5.npz'))
    sd = golden5_checkpoint(ck, golden_dir)
    lp_tol = 1e-4 if ck in ('tl', 'tl2') else 2e-5         # the trained-like log-softmax spans ~40 (a peaky map)
    for gname, (h, w) in GEOMS.items():
        assert U.get_optimal_out_size((h, w)) == NET[gname] == NET_SIZES[gname]
        frames = golden5_frames(g, gname)
        taps = {}
        maps = U.saliency_u8(sd, frames, taps)
        for i in range(frames.shape[0]):
            tag = '%s_%s_%d' % (ck, gname, i)
            t = taps['frames'][i]
            assert t['input'].shape[-2:] == NET[gname]
            ref8, idx = golden5_u8(g, ck, gname, i)
            d = np.abs(maps[:, :, i][idx].astype(int) - ref8.astype(int))
            assert d.max() <= 1 and (d > 0).mean() < 2e-3, tag
            if i == 0:
                lp = torch.log_softmax(t['pre'].reshape(1, -1), 1).reshape(h, w).numpy()
                assert np.abs(lp[np.ix_(*grid(h, w))] - g['logp_' + tag]).max() < lp_tol, tag
                ref = g['adapt_' + tag]
                a = t['adapt'][0].numpy()
                assert np.allclose(a[np.ix_(*grid(a.shape[0], a.shape[1], 2))], ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max()), tag


# fp32 oracle against its own float64 evaluation, elementwise max |fp32 - fp64| / max|fp64| over every tap and the eleven geometries.
# Measured (one synth.blob_frames frame per geometry): carrier 3.6e-5 (feat_1x), reference-initialised 1.3e-4 (pre, dec, post_cnn);
# the bounds are about twice that.  u8 maps: one grey level on at most 0.02 % / 0.4 % of the pixels.
_F64_BOUND = {'carrier': (8e-5, 1e-3), 'ri': (2.5e-4, 8e-3)}


@pytest.mark.parametrize('ck', ['carrier', 'ri'])
def test_fp32_oracle_agrees_with_its_float64_evaluation_at_eleven_geometries(golden_dir, ck):
    """The float64 mode evaluates the same operations: it agrees with the fp32 oracle within the fp32 rounding (bound measured, above),
    keeps every tap in float64, and the quantisation to u8 stays the reference's fp32 one."""
    from retargetvid_amd import synth, weights
    torch.set_num_threads(4)
    sd = weights.make_synthetic_state_dict(0) if ck == 'carrier' else golden5_checkpoint('ri', golden_dir)
    bound, u8_frac = _F64_BOUND[ck]
    for gname, (h, w) in ELEVEN.items():
        fr = synth.blob_frames(1, h, w, seed=h * w)
        a, b = {}, {}
        m32 = U.saliency_u8(sd, fr, a)
        m64 = U.saliency_u8(sd, fr, b, dtype=torch.float64)
        ta, tb = a['frames'][0], b['frames'][0]
        assert tb['input'].shape[-2:] == NET_SIZES[gname]
        assert np.abs(ta['input'].numpy() - tb['input'].numpy()).max() < 1e-6, gname
        for k in ('feat_4x', 'feat_2x', 'feat_1x', 'post_cnn', 'dec', 'adapt', 'pre'):
            assert tb[k].dtype == torch.float64 and ta[k].dtype == torch.float32, k
            r = tb[k].numpy()
            e = np.abs(ta[k].numpy() - r).max() / np.abs(r).max()
            assert e <= bound, (gname, k, e)
        d = np.abs(m32.astype(int) - m64.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < u8_frac, gname
    pre = torch.randn(1, 20, 30, dtype=torch.float64)
    assert np.array_equal(U.quantise_u8(pre), U.quantise_u8(pre.float()))
