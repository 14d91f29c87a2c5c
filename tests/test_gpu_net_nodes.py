"""-m gpu: the saliency network NODE BY NODE (svc_debug_run_node: one stage of forward_chunk on the test's input, everything it may
write pre-filled with NaN) against the float64 node oracle (oracle/unisal_nodes_ref.py), on both matrix pipes.

(a) exact cases: operands on dyadic grids (tests/net_node_cases.py), every product and partial sum an fp32 number in any order
    (asserted on the float64 side) -- the device must give the float64 value bit for bit, at all eleven geometries.
(b) full-mantissa cases: |device - value| <= C_GATE u bound at EVERY element, the constant measured on the fp32 pipe
    (profiles/net_node_error.md) and the same for the split-bf16 pipe, whose claim is fp32-class arithmetic.
(c) the door launches what the pass launches: the graph walked node by node on the device's own outputs ends in the bytes of one
    saliency() call's DEC and PRE taps."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import net_node_cases as C
from oracle import unisal_nodes_ref as N
from retargetvid_amd import ops
from test_oracle_unisal import ELEVEN, NET_SIZES

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

PIPES = ('bf16x6', 'f32')


def _engine(pipe, sd=None, layers=None):
    old = os.environ.get('SVC_MX')
    os.environ['SVC_MX'] = pipe
    try:
        eng = ops.Engine(sd) if layers is None else ops.Engine.from_layers(layers)
    finally:
        if old is None:
            os.environ.pop('SVC_MX', None)
        else:
            os.environ['SVC_MX'] = old
    assert eng.matrix_pipe() == pipe
    return eng


@pytest.fixture(scope='module')
def engines():
    """Handles by (checkpoint or 'exact', pipe), made on first use and closed with the module."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    made = {}

    def get(ck, pipe):
        if (ck, pipe) not in made:
            made[(ck, pipe)] = _engine(pipe, layers=C.exact_layers()) if ck == 'exact' else _engine(pipe, sd=C.checkpoint(ck)[0])
        return made[(ck, pipe)]
    yield get
    for e in made.values():
        e.close()


def _assert_rest_is_fill(rest, where):
    assert (rest == C.FILL).all(), (where, 'the part of the row the node does not own was written')


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
EXACT_CASES = [(g, 3) for g in ELEVEN] + [('16x9', 1), ('16x9', 4)]       # M = n H5 W5 = 104 / 312 / 416 at 256x416


@pytest.mark.parametrize('gname,n', EXACT_CASES)
def test_exact_cases_equal_the_float64_value_bit_for_bit(engines, gname, n):
    """Every node but the front and the smoothing, grid operands, frames of different content: device == float64 value at every
    element on both pipes, nothing left unwritten, the un-owned part of a row still the fill."""
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    layers = C.exact_layers()
    for i, node in enumerate(C.MAIN_NODES):
        ref = N.NodeRef(layers, bounds=False, track=True)
        in0, in1 = C.exact_inputs(node, n, NH, NW, seed=1000 * n + 31 * i + NH)
        value, _ = ref.run(node, in0, in1)
        ok, worst = C.budget_ok(ref)
        assert ok, (node, 'a partial sum may not be an fp32 number', worst)
        for pipe in PIPES:
            where = (gname, n, node, pipe)
            dev, rest = C.run_device(engines('exact', pipe), node, n, h, w, NH, NW, in0, in1)
            assert not np.isnan(dev).any(), (where, 'unwritten elements', int(np.isnan(dev).sum()), np.argwhere(np.isnan(dev))[:4].tolist())
            bad = dev.astype(np.float64) != value
            assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(dev - value).max()))
            _assert_rest_is_fill(rest, where)


@pytest.mark.parametrize('stage', ['first', 'last'])
@pytest.mark.parametrize('bits', C.WIDE_BITS)
def test_wide_operand_exact_cases_need_every_kept_plane_pair(bits, stage):
    """Operands of (10, 10), (18, 3) and (3, 18) significant bits in one 1x1 stage of every node, the other stages passing values
    through (net_node_cases.wide_layers): m.m, m.h / l.h and h.m / h.l carry value, and the device must still equal float64 bit
    for bit on both pipes -- a dropped or mis-indexed plane pair shows.  256x416 at n = 3 (a row-tile remainder), 320x320 at n = 1."""
    xb, wb = bits
    layers = C.wide_layers(xb, wb, stage)
    engs = {pipe: _engine(pipe, layers=layers) for pipe in PIPES}
    try:
        for gname, n in (('16x9', 3), ('1x1', 1)):
            h, w = ELEVEN[gname]
            NH, NW = NET_SIZES[gname]
            for i, node in enumerate(C.WIDE_NODES[stage]):
                ref = N.NodeRef(layers, bounds=False, track=True)
                in0, in1 = C.wide_inputs(node, n, NH, NW, xb, seed=77 * i + NH + n)
                value, _ = ref.run(node, in0, in1)
                ok, worst = C.budget_ok(ref)
                assert ok, (node, 'a partial sum may not be an fp32 number', worst)
                for pipe in PIPES:
                    where = (bits, stage, gname, n, node, pipe)
                    dev, rest = C.run_device(engs[pipe], node, n, h, w, NH, NW, in0, in1)
                    assert not np.isnan(dev).any(), (where, 'unwritten elements', int(np.isnan(dev).sum()))
                    bad = dev.astype(np.float64) != value
                    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(dev - value).max()))
                    _assert_rest_is_fill(rest, where)
    finally:
        for e in engs.values():
            e.close()


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
def _gate(dev, value, bound, c, where):
    assert np.isfinite(dev).all(), (where, 'non-finite or unwritten elements', int((~np.isfinite(dev)).sum()))
    d = np.abs(dev.astype(np.float64) - value)
    out = d > c * C.U32 * bound
    assert not out.any(), (where, int(out.sum()), np.argwhere(out)[:4].tolist(), C.error_ratio(dev, value, bound))


def _f18_clamps(ck, in0, dev, where):
    """Where the float64 pre-activation is clear of the clamp by more than the gate, the device value is the clamp itself."""
    l = C.checkpoint(ck)[2].L['f18']
    x, wt = in0.astype(np.float64), l['w'].astype(np.float64)
    pre, bound = x @ wt.T + l['b'], np.abs(x) @ np.abs(wt).T + np.abs(l['b'])
    tol = C.gate_c('f18') * C.U32 * bound
    assert (dev[pre < -tol] == 0.0).all(), (where, 'f18 below the clamp')
    assert (dev[pre > 6.0 + tol] == 6.0).all(), (where, 'f18 above the clamp')


@pytest.mark.parametrize('gname', list(ELEVEN))
@pytest.mark.parametrize('ck', ['tl', 'ri'])
def test_every_node_within_the_per_element_bound_on_the_oracles_activations(engines, ck, gname):
    """Each node on the float64 oracle's own activations (rounded to fp32) of the goldens' frames (all of a geometry in one batch): |device - value| <= C_GATE u
    bound elementwise on both pipes (C = net_node_cases.gate_c: at most C_GATE; smoothing: C_SMOOTH), outputs finite, f18 exactly 0 / 6 beyond the clamp, un-owned row parts
    still the fill.  The front runs from the uint8 frames and is gated against the float64 evaluation of stem + features.1 from the
    fp32 ORACLE's network input (oracle.unisal_ref.preprocess), not from the device's own TAP_INPUT: stricter, since the device's
    LANCZOS and normalisation must then give the oracle's input (test_gpu_geometries asserts they do, bit for bit) -- a
    resampling disagreement would show here as an error the bound does not account for."""
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    frames = C.golden_frames(ck, gname)
    for node, in0, in1, value, bound in C.oracle_activation_cases(ck, frames, h, w, NH, NW, C.MAIN_NODES + ['smooth']):
        for pipe in PIPES:
            where = (ck, gname, node, pipe)
            dev, rest = C.run_device(engines(ck, pipe), node, len(frames), h, w, NH, NW, in0, in1)
            _gate(dev, value, bound, C.gate_c(node), where)
            _assert_rest_is_fill(rest, where)
            if node == 'f18':
                _f18_clamps(ck, in0, dev, where)
    value, bound = C.checkpoint(ck)[2].run('front', C.network_input(frames, torch.float32))
    for pipe in PIPES:
        dev, _ = C.run_device(engines(ck, pipe), 'front', len(frames), h, w, NH, NW, frames)
        _gate(dev, value, bound, C.gate_c('front'), (ck, gname, 'front', pipe))


@pytest.mark.parametrize('gname', C.ADVERSARIAL_GEOMS)
def test_every_node_within_the_per_element_bound_on_adversarial_inputs(engines, gname):
    """Two kinds, three frames each, the same elementwise gate: N(0, 1) inputs with 1 % of the entries x100 and 10 % exact zeros;
    inputs solved so that pre-activations sit at 0 and at 6 ahead of the node's first ReLU6 (net_node_cases.straddling_inputs)."""
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    ref = C.checkpoint('tl')[2]
    cases = [('outliers', node) + C.adversarial_inputs(node, 3, NH, NW, C.adversarial_seed(node, NH)) for node in C.MAIN_NODES]
    cases += [('straddling', node) + C.straddling_inputs(ref, node, 3, NH, NW, C.adversarial_seed(node, NH)) for node in N.PW_NODES]
    for kind, node, in0, in1 in cases:
        value, bound = ref.run(node, in0, in1)
        for pipe in PIPES:
            where = ('tl', gname, kind, node, pipe)
            dev, rest = C.run_device(engines('tl', pipe), node, 3, h, w, NH, NW, in0, in1)
            _gate(dev, value, bound, C.gate_c(node), where)
            _assert_rest_is_fill(rest, where)
            if node == 'f18':
                _f18_clamps('tl', in0, dev, where)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pipe', PIPES)
@pytest.mark.parametrize('gname', ['16x9', '1x1', 'port'])
def test_the_graph_walked_through_the_door_gives_the_bytes_of_the_pass(engines, gname, pipe):
    """From the front on, each node fed the device's own previous output: DEC and PRE at the end are the taps of one saliency()
    call on the same frames, byte for byte -- the door and forward_chunk launch the same kernels on the same buffers."""
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    eng = engines('tl', pipe)
    frames = C.golden_frames('tl', gname)[:2]
    n = len(frames)
    eng.saliency(torch.from_numpy(frames).cuda())
    dec = np.stack([eng.tap(ops.TAP_DEC, i, (NH // 8, NW // 8, 64)) for i in range(n)])
    pre = np.stack([eng.tap(ops.TAP_PRE, i, (h, w)) for i in range(n)])
    priors = np.stack([eng.tap(ops.TAP_FEAT1X, i, (NH // 32, NW // 32, 1296)) for i in range(n)])[..., 1280:]
    run = lambda node, a, b=None: C.run_device(eng, node, n, h, w, NH, NW, a, b)[0]
    x = run('front', frames)
    for idx in range(2, 18):
        if idx == 7:
            f4x = run('f4x', x)
        if idx == 14:
            f2x = run('f2x', x)
        x = run('block%d' % idx, x)
    pc = run('post_cnn', np.concatenate((run('f18', x), priors), axis=3))
    u2 = run('us2', pc, run('skip_2x', f2x))
    got_dec = run('post_us2', u2, run('skip_4x', f4x))
    assert np.array_equal(got_dec.view(np.uint32), dec.view(np.uint32)), (gname, pipe, 'DEC')
    got_pre = run('smooth', run('adapt', got_dec))
    assert np.array_equal(got_pre.view(np.uint32), pre.view(np.uint32)), (gname, pipe, 'PRE')
    # the pass after the door: the workspace the door filled gives the same bytes again
    eng.saliency(torch.from_numpy(frames).cuda())
    assert np.array_equal(np.stack([eng.tap(ops.TAP_PRE, i, (h, w)) for i in range(n)]).view(np.uint32), pre.view(np.uint32))


def test_the_door_refuses_invalid_arguments(engines):
    eng = engines('tl', 'f32')
    x = np.zeros((1, 8, 13, 320), np.float32)
    with pytest.raises(Exception, match='unknown node'):
        eng.run_node(99, 1, 140, 250, x, None, (8, 13, 1296))
    with pytest.raises(Exception, match='frames'):
        eng.run_node(ops.NODE_F18, 0, 140, 250, x, None, (8, 13, 1296))
    with pytest.raises(Exception, match='frames'):
        eng.run_node(ops.NODE_F18, 33, 140, 250, np.zeros((33, 8, 13, 320), np.float32), None, (8, 13, 1296))
    with pytest.raises(Exception, match='skip input'):
        eng.run_node(ops.NODE_US2, 1, 140, 250, np.zeros((1, 8, 13, 256), np.float32), None, (16, 26, 128))
    with pytest.raises(Exception, match='too small'):
        eng.run_node(ops.NODE_F18, 1, 140, 250, x, None, (8, 13, 1280))
    # the map nodes (26, 27): the ids behind them are still unknown, and they need room for both planes
    logit = np.zeros((1, 32, 52), np.float32)
    for node in (28, 29, 0, -1):
        with pytest.raises(Exception, match='unknown node'):
            eng.run_node(node, 1, 140, 250, logit, None, (2, 140, 250))
    for node in (ops.NODE_MAP, ops.NODE_MAP_PROFILE):
        with pytest.raises(Exception, match='too small'):
            eng.run_node(node, 1, 140, 250, logit, None, (140, 250))
        with pytest.raises(Exception, match='frames'):
            eng.run_node(node, 0, 140, 250, logit, None, (2, 140, 250))
        with pytest.raises(Exception, match='frames'):
            eng.run_node(node, 33, 140, 250, np.zeros((33, 32, 52), np.float32), None, (2, 140, 250))
        got = eng.run_node(node, 1, 140, 250, logit, None, (2, 140, 250))
        assert got.shape == (1, 2, 140, 250) and (got[0, 0] == 0.0).all() and (got[0, 1] == 255.0).all(), node
