"""TransNet V1 on the device layer by layer (svc_debug_transnet_tap) against the float64 restatement of the reference's graph
(oracle/transnet_ref.forward(..., torch.float64, taps=True); PARITY UNPINNED against TensorFlow, see its header).

Why not only P: with the test weights the softmax output is saturated (a |dP| gate of 1e-4 allows a logit error of ~7e-3 at the
median), the max-pools hide most of a cell's values (and the last row of the odd-height maps entirely), and the default weights and
inputs have no exact ReLU zeros at scale, no large exponents, no window shorter than the dilation-8 reach.  So every layer is checked,
at every position, for four weight variants (R.VARIANTS), five input kinds (R.INPUTS), window lengths 1 .. 100 and 3 windows in one
call, on every form of the cells (PIPES).

Gate per tap: |device - float64| <= ATOL * max|float64| + RTOL * |float64|, ATOL / RTOL per pipe class in GATES, set from the MI355X
measurement in profiles/transnet_layer_error.md (tools/transnet_error_report.py) with the headroom stated there."""
import functools
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import transnet_ref as R
from retargetvid_amd import _lib, transnetv1_handler as Hd

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

# (ATOL, RTOL, logit tolerance); a cell's and a pool's max|ref| is that of the cell's pre-ReLU values.  Measured on the MI355X
# (profiles/transnet_layer_error.md), largest over every layer, variant and case: bf16x6 with every tile knob 2.1e-6 of max|ref|, f32
# 3.8e-6 (its fp32 MFMA sums the 27 taps in another order), logits 1.1e-5; bf16x3 1.8e-4, logits 3.3e-4.  ATOL = RTOL = 1e-5 for the
# fp32 class (2.6x the f32 pipe's maximum; 5e-6 left it 1.3x), 5e-4 for bf16x3 (2.8x); logits 4e-5 / 1e-3 (3.6x / 3x).
GATES = {'fp32': (1e-5, 1e-5, 4e-5), 'bf16x3': (5e-4, 5e-4, 1e-3)}
DENSE_GATE = 2e-6                 # Dense(256) against float64 Dense on the device's own pool-3 tap (fp32 MFMA, 4 608 products, 8 K parts)

PIPES = {                          # name: (environment when the handle is created, matrix pipe, config()[1:])
    'default': ({}, 'bf16x6', [3, 1]),
    'm16_2': ({'SVC_SHOT_M16': '2'}, 'bf16x6', [2, 1]),
    'm16_4_xcd0': ({'SVC_SHOT_M16': '4', 'SVC_SHOT_XCD': '0'}, 'bf16x6', [4, 0]),
    'f32': ({'SVC_SHOT_MX': 'f32'}, 'f32', [3, 1]),
    'bf16x3': ({'SVC_SHOT_MX': 'bf16x3'}, 'bf16x3', [3, 1]),
}
LENGTHS = (1, 2, 8, 9, 16, 17, 37, 100)
MULTI = (17, ('video', 'zeros', 'gradient'))      # 3 windows of 17 frames in one call, three kinds of content
CELLS = ['cell%d' % i for i in range(1, 7)]
LAYERS = ['input'] + CELLS + ['pool1', 'pool2', 'pool3', 'dense']          # index = SVC_SHOT_TAP_*


def gates(pipe):
    return GATES['bf16x3' if PIPES[pipe][1] == 'bf16x3' else 'fp32']


def cases(variant):
    """[(frames [nw, T, 27, 48, 3], label)]: every length once, the input kind cycling with the variant so that every variant sees
    all five kinds and every kind several lengths; then 3 windows in one call."""
    vi = R.VARIANTS.index(variant)
    out = []
    for i, T in enumerate(LENGTHS):
        kind = R.INPUTS[(i + vi) % len(R.INPUTS)]
        out.append((R.frames(kind, T, 100 * vi + i)[None], '%s T=%d' % (kind, T)))
    T, kinds = MULTI
    out.append((np.stack([R.frames(k, T, 100 * vi + 50 + j) for j, k in enumerate(kinds)]), '3 windows T=%d' % T))
    return out


@functools.lru_cache(maxsize=None)
def oracle(variant):
    """(state dict, [(frames, label, float64 taps)]) -- computed once per variant and shared by every pipe."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = R.variant_state_dict(variant)
    return sd, [(fr, label, R.forward(sd, fr, torch.float64, taps=True)[1]) for fr, label in cases(variant)]


def make_net(pipe, sd):
    env, mx, cfg = PIPES[pipe]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = Hd.ShotTransNet(Hd.ShotTransNetParams(), weights=sd)       # the knobs are read when the handle is created
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert net.matrix_pipe() == mx and net.config()[1:] == cfg, (pipe, net.matrix_pipe(), net.config())
    return net


def load(net, sd):
    blob = np.ascontiguousarray(Hd._weights.pack_transnet_blob(sd), np.float32)
    _lib.check(net.eng.lib.svc_transnet_load(net.eng._h, blob.ctypes.data_as(Hd.ctypes.c_void_p), blob.size))


@pytest.fixture(scope='module')
def nets():
    made = {}

    def get(pipe, variant):
        if pipe not in made:
            made[pipe] = [make_net(pipe, oracle(variant)[0]), variant]
        elif made[pipe][1] != variant:
            load(made[pipe][0], oracle(variant)[0])
            made[pipe][1] = variant
        return made[pipe][0]
    yield get
    for n, _ in made.values():
        n.close()


def within(got, ref, atol, rtol, scale=None):
    """Gate mask and the largest |d| / max|ref|."""
    ref = ref.astype(np.float64)
    m = np.abs(ref).max() if scale is None else scale
    d = np.abs(got.astype(np.float64) - ref)
    return d <= atol * m + rtol * np.abs(ref), float(d.max() / m) if m > 0 else float(d.max())


def pool2(x):
    """MaxPool3D (1, 2, 2), VALID, on [..., H, W, C] (the odd last row / column dropped)."""
    h, w = x.shape[-3] // 2, x.shape[-2] // 2
    x = x[..., :2 * h, :2 * w, :]
    return x.reshape(x.shape[:-3] + (h, 2, w, 2, x.shape[-1])).max((-4, -2))


def tap_scale(ref, layer, s):
    """max|ref| of a tap's gate: a cell's and a pool's scale is that of the cell's pre-ReLU values (what the kernel computes; the
    ReLU only clamps them), the others their own."""
    if layer.startswith('cell') or layer.startswith('pool'):
        c = int(layer[4:]) if layer.startswith('cell') else 2 * int(layer[4:])
        return float(np.abs(ref['pre%d' % c][:, s]).max())
    return float(np.abs(ref[layer][:, s]).max())


def check_layers(net, sd, pipe, fr, ref, label, rows=None, frames_of=None):
    """Every tap of the device against the float64 taps (on the frames each layer computes: frames_of(layer) -> slice), the exact
    ReLU zeros, the pools bit for bit from the device's own cells, Dense(256) on the device's own pool 3.  Returns the device's taps."""
    atol, rtol, _ = gates(pipe)
    sel = frames_of or (lambda layer: slice(None))
    dev = {}
    for li, layer in enumerate(LAYERS):
        got = net.debug_tap(fr, li, rows)
        assert got.shape == ref[layer].shape, (label, layer, got.shape)
        dev[layer] = got
        s = sel(layer)
        g, r = got[:, s], ref[layer][:, s]
        if layer != 'dense':
            ok, e = within(g, r, atol, rtol, tap_scale(ref, layer, s))
            assert ok.all(), (pipe, label, layer, 'error %.3g of max|ref|' % e, int((~ok).sum()))
        if layer.startswith('cell'):
            pre = ref['pre' + layer[4:]][:, s]
            lim = atol * tap_scale(ref, layer, s) + rtol * np.abs(pre)
            assert (g[pre < -lim] == 0).all(), (pipe, label, layer, 'a value the float64 ReLU zeroes is not 0')
            assert (g[pre > lim] > 0).all(), (pipe, label, layer, 'a value the float64 ReLU keeps is 0')
        if layer.startswith('pool'):
            cell = dev['cell%d' % (2 * int(layer[4:]))][:, s]
            assert np.array_equal(g, pool2(cell)), (pipe, label, layer, 'not the 2x2 maximum of the device\'s own cell')
    p3 = dev['pool3'][:, sel('dense')].astype(np.float64)
    d64 = np.maximum(p3.reshape(p3.shape[:2] + (-1,)) @ sd['TransNet/dense/kernel'].astype(np.float64)
                     + sd['TransNet/dense/bias'].astype(np.float64), 0)
    ok, e = within(dev['dense'][:, sel('dense')], d64, DENSE_GATE, DENSE_GATE)
    assert ok.all(), (pipe, label, 'Dense(256) on the device\'s pool 3: %.3g of max|ref|' % e)
    ok, e = within(dev['dense'][:, sel('dense')], ref['dense'][:, sel('dense')], atol, rtol)
    assert ok.all(), (pipe, label, 'dense', 'error %.3g of max|ref|' % e)
    return dev


def check_logits(pipe, P, ref, label):
    """log(P / (1 - P)) of the device against the float64 logit1 - logit0 where P64 is in [1e-3, 1 - 1e-3]; the float32 rounding of
    P itself allows 2^-24 / (1 - P) per ulp -- eight of them are added to the tolerance."""
    p64 = ref['P']
    band = (p64 >= 1e-3) & (p64 <= 1 - 1e-3)
    if not band.any():
        return 0
    p = P[band].astype(np.float64)
    got = np.log(p / (1 - p))
    want = (ref['logits'][..., 1] - ref['logits'][..., 0])[band]
    tol = gates(pipe)[2] + 8 * 2.0 ** -24 / (1 - p)
    d = np.abs(got - want)
    assert (d <= tol).all(), (pipe, label, 'logit error %.3g' % d.max())
    return int(band.sum())


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('pipe', list(PIPES))
def test_every_layer_every_position_against_float64(nets, pipe, variant):
    sd, refs = oracle(variant)
    net = nets(pipe, variant)
    in_band = 0
    for fr, label, ref in refs:
        check_layers(net, sd, pipe, fr, ref, label)
        P = net.predict_raw(fr)
        ok, e = within(P, ref['P'], *gates(pipe)[:2], scale=1.0)
        assert ok.all(), (pipe, label, 'P', e)
        in_band += check_logits(pipe, P, ref, label)
    if variant != 'loud':                                            # the loud network's P is saturated by design
        assert in_band > 50, (variant, in_band)


KEPT = [(100, (25, 75)), (100, (0, 1)), (100, (99, 100)), (100, (3, 12)), (100, (40, 97)), (37, (5, 30))]


def computed_frames(layer, T, r0, r1):
    """The frames svc_transnet_predict_rows must compute for kept rows [r0, r1), derived here: the last cell on [r0, r1), every cell
    in front of it 8 frames more to either side (its largest dilation), clipped to the window; cell 1 and the input on every frame; a
    pool on its block's last cell's frames; Dense(256) on the kept rows."""
    if layer in ('input', 'cell1'):
        return slice(0, T)
    if layer == 'dense':
        return slice(r0, r1)
    i = int(layer[4:]) if layer.startswith('cell') else 2 * int(layer[4:])
    return slice(max(0, r0 - 8 * (6 - i)), min(T, r1 + 8 * (6 - i)))


@pytest.mark.parametrize('pipe', list(PIPES))
def test_kept_rows_against_float64(nets, pipe):
    """svc_transnet_predict_rows at odd row ranges: every layer on the frames it computes, and the kept rows of P, against the float64
    oracle (the existing test compares the kept rows with the full pass only)."""
    sd, refs = oracle('seed0')
    net = nets(pipe, 'seed0')
    by_T = {fr.shape[1]: (fr, label, ref) for fr, label, ref in refs if fr.shape[0] == 1}
    for T, (r0, r1) in KEPT:
        fr, label, ref = by_T[T]
        check_layers(net, sd, pipe, fr, ref, '%s rows %d..%d' % (label, r0, r1), rows=(r0, r1),
                     frames_of=lambda layer: computed_frames(layer, T, r0, r1))
        P = net.predict_raw_device(torch.from_numpy(fr).cuda(), rows=(r0, r1)).cpu().numpy()[:, r0:r1]
        ok, e = within(P, ref['P'][:, r0:r1], *gates(pipe)[:2], scale=1.0)
        assert ok.all(), (pipe, T, r0, r1, e)


def test_the_variants_do_what_they_are_for():
    """sparse: at least 70 % of every cell's float64 outputs are exact zeros over its cases; loud: the last cell reaches ~1e3;
    calibrated: most P of its cases lie in [0.05, 0.95]."""
    _, refs = oracle('sparse')
    for c in CELLS:
        assert np.mean(np.concatenate([(ref[c] == 0).ravel() for _, _, ref in refs])) >= 0.7, c
    _, refs = oracle('loud')
    assert max(np.abs(ref['cell6']).max() for _, _, ref in refs) > 500
    _, refs = oracle('calibrated')
    P = np.concatenate([ref['P'].ravel() for _, _, ref in refs])
    assert np.mean((P >= 0.05) & (P <= 0.95)) > 0.9


def test_tap_door_errors(nets):
    """svc_debug_transnet_tap refuses an unknown layer, a buffer that is too small and more windows than one pass holds; a handle without
    weights refuses it too."""
    import ctypes
    net = nets('default', 'seed0')
    fr = torch.zeros((1, 4, 27, 48, 3), dtype=torch.uint8, device='cuda')
    out = np.empty(4 * 27 * 48 * 64, np.float32)
    lib, h, vp = net.eng.lib, net.eng._h, ctypes.c_void_p
    assert lib.svc_debug_transnet_tap(h, vp(fr.data_ptr()), 1, 4, 0, 4, 1, out.ctypes.data_as(vp), out.size) == 0
    for layer, cap in ((11, out.size), (-1, out.size), (1, out.size - 1)):
        assert lib.svc_debug_transnet_tap(h, vp(fr.data_ptr()), 1, 4, 0, 4, layer, out.ctypes.data_as(vp), cap) == -1, layer
    many = torch.zeros((17, 100, 27, 48, 3), dtype=torch.uint8, device='cuda')     # 16 windows of 100 per pass on bf16x6
    big = np.empty(17 * 100 * 256, np.float32)
    assert lib.svc_debug_transnet_tap(h, vp(many.data_ptr()), 17, 100, 0, 100, 10, big.ctypes.data_as(vp), big.size) == -1
    assert b'one pass' in lib.svc_last_error()
    from retargetvid_amd import ops
    eng = ops.Engine(seed=0)
    try:
        assert eng.lib.svc_debug_transnet_tap(eng._h, vp(fr.data_ptr()), 1, 4, 0, 4, 1, out.ctypes.data_as(vp), out.size) == -1
    finally:
        eng.close()
