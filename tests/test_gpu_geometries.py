"""-m gpu: the HIP network at all eleven network input sizes that get_optimal_out_size can select for a saliency map of at most
250 px (tests/test_oracle_unisal.py: ELEVEN), every tap of every frame against the FLOAT64 oracle, with the gates of
tests/test_gpu_parity.py (_TOL, _TAPS; imported, not copied).  The fp32 oracle is itself up to ~1e-4 of max|ref| off its float64
evaluation (test_fp32_oracle_agrees_with_its_float64_evaluation_at_eleven_geometries), so against the float64 one the device's own
error is what is measured.  u8 maps against the fp32 oracle (the reference's arithmetic) and the reference model's maps
(unisal_golden.npz / golden2-4 at the three geometries those cover, golden5 at the other eight: whole maps for tl / tl2, grid
samples for nc / ri)."""
import functools
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import unisal_ref as U
from retargetvid_amd import ops, synth, weights
from test_gpu_parity import _TAPS, _TOL
from test_oracle_unisal import ELEVEN, NET_SIZES, golden5_checkpoint, golden5_frames, golden5_u8

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OLD = ('16x9', '4x3', 'port')                 # the geometries of golden2-4
# the carrier checkpoint (conftest synthetic_sd) is a synthetic one: the gates of the other synthetic checkpoint, nc
GATES = dict(_TOL, carrier=_TOL['nc'])


@functools.lru_cache(maxsize=None)
def _npz(name):
    return np.load(os.path.join(GOLDEN, name))


@functools.lru_cache(maxsize=None)
def _checkpoint(ck):
    return weights.make_synthetic_state_dict(0) if ck == 'carrier' else golden5_checkpoint(ck, GOLDEN)


def _frames_and_reference_maps(ck, gname):
    """Frames of (checkpoint, geometry) and the reference model's u8 maps of them: per frame (map, index of the map's pixels it
    holds) -- the whole map, or every other row and column (golden5, nc / ri) -- or None where no golden holds them."""
    h, w = ELEVEN[gname]
    whole = np.ix_(np.arange(h), np.arange(w))
    if gname not in OLD:
        g = _npz('unisal_golden5.npz')
        fr = golden5_frames(g, gname)
        return fr, None if ck == 'carrier' else [golden5_u8(g, ck, gname, i) for i in range(len(fr))]
    if ck == 'carrier':
        if gname == '16x9':
            g = _npz('unisal_golden.npz')
            return g['frames'][:2], [(g['smaps_u8'][:, :, i], whole) for i in range(2)]
        return synth.blob_frames(2, h, w, seed=h + w), None
    g = _npz({'tl': 'unisal_golden3.npz', 'tl2': 'unisal_golden4.npz'}.get(ck, 'unisal_golden2.npz'))
    fr = g['frames_' + gname]
    return fr, [(g['u8_%s_%s_%d' % (ck, gname, i)], whole) for i in range(len(fr))]


@functools.lru_cache(maxsize=None)
def _oracle(ck, gname):
    """(frames, reference-model maps, fp32 oracle maps [n,h,w], fp32 network inputs [n,NH,NW,3], float64 taps per frame)."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = _checkpoint(ck)
    fr, gold = _frames_and_reference_maps(ck, gname)
    t32, t64 = {}, {}
    m32 = U.saliency_u8(sd, fr, t32)
    U.saliency_u8(sd, fr, t64, dtype=torch.float64)
    inputs = np.stack([t['input'][0].permute(1, 2, 0).numpy() for t in t32['frames']])
    taps = []
    for t in t64['frames']:
        d = {key: t[key][0].permute(1, 2, 0).numpy() for key, _, _, _ in _TAPS}
        d['pre'] = t['pre'][0].numpy()
        gm = U.gaussian_maps(torch.as_tensor(np.asarray(sd['coarse_gaussians_salicon'])), d['feat_1x'].shape[0], d['feat_1x'].shape[1],
                             dtype=torch.float64)
        d['gauss'] = gm.permute(1, 2, 0).numpy()
        taps.append(d)
    return fr, gold, np.transpose(m32, (2, 0, 1)), inputs, taps


def _engine(sd, pipe):
    old = os.environ.get('SVC_MX')
    os.environ['SVC_MX'] = pipe
    try:
        eng = ops.Engine(sd)
    finally:
        if old is None:
            os.environ.pop('SVC_MX', None)
        else:
            os.environ['SVC_MX'] = old
    assert eng.matrix_pipe() == pipe
    return eng


@pytest.mark.parametrize('ck,pipe', [('carrier', 'bf16x6'), ('nc', 'bf16x6'), ('ri', 'bf16x6'), ('tl', 'bf16x6'), ('tl2', 'bf16x6'),
                                     ('tl', 'f32')])
def test_network_every_tap_at_eleven_geometries_against_float64(ck, pipe):
    """Network input bit-exact against the fp32 oracle; FEAT4X, FEAT2X, FEAT1X (1280 channels), POSTCNN, DEC and PRE against the
    float64 oracle (elementwise atol * max|ref| + 1e-4 |ref| and the mean bound of _TOL); the 16 Gaussian prior channels of FEAT1X
    against their float64 evaluation; u8 maps within one grey level on less than the _TOL fraction of the pixels against the fp32
    oracle and the reference model."""
    atol_f, mean_f, u8_frac = GATES[ck]
    eng = _engine(_checkpoint(ck), pipe)
    try:
        for gname, (h, w) in ELEVEN.items():
            NH, NW = NET_SIZES[gname]
            fr, gold, ref32, inputs, taps64 = _oracle(ck, gname)
            maps = eng.saliency(torch.from_numpy(fr).cuda()).cpu().numpy()
            for i in range(len(fr)):
                where = (ck, pipe, gname, i)
                assert np.array_equal(eng.tap(ops.TAP_INPUT, i, (NH, NW, 3)), inputs[i]), where
                f1 = None
                for key, tap, div, ch in _TAPS + (('pre', 'TAP_PRE', None, None),):
                    got = eng.tap(getattr(ops, tap), i, (NH // div, NW // div, ch) if div else (h, w))
                    if key == 'feat_1x':
                        f1, got = got, got[:, :, :1280]
                    ref = taps64[i][key]
                    assert got.shape == ref.shape, (where, key)
                    scale = float(np.abs(ref).max())
                    d = np.abs(got.astype(np.float64) - ref)
                    assert (d <= atol_f * scale + 1e-4 * np.abs(ref)).all(), (where, key, float(d.max() / scale))
                    assert d.mean() <= mean_f * scale, (where, key, float(d.mean() / scale))
                # the Gaussian priors (emulated fp32 torch.linspace of H/32 and W/32 points): fp32 rounding only
                gref = taps64[i]['gauss']
                assert np.abs(f1[:, :, 1280:] - gref).max() <= 1e-5 * np.abs(gref).max(), (where, 'gauss')
                whole = np.ix_(np.arange(h), np.arange(w))
                for name, ref8 in (('oracle', (ref32[i], whole)), ('reference', None if gold is None else gold[i])):
                    if ref8 is None:
                        continue
                    r8, idx = ref8
                    du = np.abs(maps[i][idx].astype(int) - r8.astype(int))
                    assert du.max() <= 1 and (du > 0).mean() < u8_frac, (where, name, int(du.max()), float((du > 0).mean()))
    finally:
        eng.close()


def test_one_handle_through_the_geometries_gives_the_bytes_of_fresh_handles(engine, synthetic_sd):
    """One handle visiting the geometries in turn (A, B, A, C, ...: plan rebuilds, LANCZOS / smoothing tables, the Gaussian-prior
    refill after every change, batches that grow and shrink at one geometry) gives the maps and the decoder and pre-softmax taps of a
    fresh handle per geometry, byte for byte."""
    names = list(ELEVEN)
    frames, fresh = {}, {}
    for gname in names:
        h, w = ELEVEN[gname]
        NH, NW = NET_SIZES[gname]
        frames[gname] = torch.from_numpy(synth.blob_frames(3, h, w, seed=7 * h + w)).cuda()
        e = ops.Engine(synthetic_sd)
        try:
            maps = e.saliency(frames[gname]).cpu().numpy()
            fresh[gname] = (maps, [e.tap(ops.TAP_DEC, i, (NH // 8, NW // 8, 64)) for i in range(3)],
                            [e.tap(ops.TAP_PRE, i, (h, w)) for i in range(3)])
        finally:
            e.close()
    order = [x for gname in names[1:] for x in (names[0], gname)] + [names[6], names[4], names[6]]
    for step, gname in enumerate(order):
        h, w = ELEVEN[gname]
        NH, NW = NET_SIZES[gname]
        n = 1 + step % 3                                        # 1, 2, 3 frames: the workspace grows, the priors are refilled
        maps, dec, pre = fresh[gname]
        got = engine.saliency(frames[gname][:n]).cpu().numpy()
        assert np.array_equal(got, maps[:n]), (step, gname, n)
        for i in range(n):
            assert np.array_equal(engine.tap(ops.TAP_DEC, i, (NH // 8, NW // 8, 64)), dec[i]), (step, gname, i)
            assert np.array_equal(engine.tap(ops.TAP_PRE, i, (h, w)), pre[i]), (step, gname, i)
