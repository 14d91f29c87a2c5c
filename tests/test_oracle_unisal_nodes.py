"""The float64 node oracle (oracle/unisal_nodes_ref.py) pinned on the CPU: its chain of nodes reproduces the graph oracle's taps, the
exact cases of tests/test_gpu_net_nodes.py fit in fp32 in any order, and the per-element gate resolves a GEMM that lost its low
plane pairs."""
import functools
import os

import numpy as np
import pytest
import torch

import net_node_cases as C
from oracle import unisal_nodes_ref as N, unisal_ref as U
from test_oracle_unisal import ELEVEN, NET_SIZES


@pytest.mark.parametrize('gname', list(ELEVEN))
@pytest.mark.parametrize('ck', ['tl', 'nc'])
def test_node_chain_reproduces_the_float64_oracle_taps(ck, gname):
    """Every node chained from the network input gives the float64 taps of oracle.unisal_ref.forward_logits to 1e-12 of each
    tensor's maximum.  The graph oracle is evaluated ON THE FOLDED WEIGHTS (identity BatchNorms carrying the folded bias,
    state_dict_from_layers): against the un-folded checkpoint the fp32 rounding of the folded weights alone is 2e-7 .. 2e-5 of the
    maximum, so 1e-12 is reachable only on the same numbers.  What is pinned is the graph: layouts, strides, taps, the split
    expansion, the resampling."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd, layers, ref = C.checkpoint(ck)
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    frames = C.golden_frames('tl', gname)[:1]
    x = U.preprocess(frames[0], dtype=torch.float64).unsqueeze(0)
    assert tuple(x.shape[-2:]) == (NH, NW)
    taps = {}
    pre = U.forward_logits(N.state_dict_from_layers(layers, sd), x, (h, w), taps)
    out = N.NodeRef(layers, ref.k41, bounds=False).chain(x.permute(0, 2, 3, 1).numpy(), (h, w), C.gaussians(sd, NH, NW))
    names = dict(feat_4x='f4x', feat_2x='f2x', feat_1x='f18', skip_2x='skip_2x', skip_4x='skip_4x', post_cnn='post_cnn', dec='post_us2')
    for key, node in names.items():
        r = taps[key].permute(0, 2, 3, 1).numpy()
        assert out[node].shape == r.shape, (key, out[node].shape, r.shape)
        assert np.abs(out[node] - r).max() <= 1e-12 * np.abs(r).max(), (ck, gname, key)
    for key, r, node in (('adapt', taps['adapt'].numpy(), 'adapt'), ('pre', pre.numpy(), 'smooth')):
        assert out[node].shape == r.shape, key
        assert np.abs(out[node] - r).max() <= 1e-12 * np.abs(r).max(), (ck, gname, key)


def test_bound_is_the_evaluator_on_absolute_values():
    """One pw stage by hand: bound = |x| |w|^T + |b|; a second stage adds its own terms to the first bound pushed through |w|;
    ReLU6 passes it through; without bounds the value is unchanged."""
    rng = np.random.RandomState(0)
    ref = N.NodeRef([])
    x, w1, b1 = rng.randn(5, 7), rng.randn(4, 7), rng.randn(4)
    v1, e1 = ref.pw(x, 0.0, w1, b1, True)
    assert np.array_equal(v1, np.clip(x @ w1.T + b1, 0, 6))
    assert np.allclose(e1, np.abs(x) @ np.abs(w1).T + np.abs(b1), rtol=1e-15)
    w2, b2 = rng.randn(3, 4), rng.randn(3)
    v2, e2 = ref.pw(v1, e1, w2, b2, False)
    assert np.allclose(e2, e1 @ np.abs(w2).T + np.abs(v1) @ np.abs(w2).T + np.abs(b2), rtol=1e-15)
    assert np.array_equal(N.NodeRef([], bounds=False).pw(v1, 0.0, w2, b2, False)[0], v2)
    assert N.grid_of(np.array([0.75, -2.5, 0.0, 8.0])) == 0.25 and N.grid_of(np.zeros(3)) == 1.0
    assert np.array_equal(N.trunc_sig(np.array([1.0 + 2.0 ** -10 + 2.0 ** -20, -3.0]), 16), [1.0 + 2.0 ** -10, -3.0])


@pytest.mark.parametrize('gname,n', [('16x9', 4), ('10x11', 1)])
def test_exact_cases_fit_fp32_in_any_order(gname, n):
    """The sufficient condition of the exact cases, on the CPU: at every stage of every node the largest sum of absolute terms spans
    fewer than 2^24 steps of the terms' grid, so each partial sum is an fp32 number whatever the order -- and so is the value."""
    NH, NW = NET_SIZES[gname]
    layers = C.exact_layers()
    for l in layers:
        if l['kind'] in ('pw', 'dw', 'adapt'):
            assert np.abs(l['w']).max() <= 0.75 and N.grid_of(l['w']) >= 0.25 and N.grid_of(l['b']) >= 0.25, l['name']
    for i, node in enumerate(C.MAIN_NODES):
        ref = N.NodeRef(layers, bounds=False, track=True)
        in0, in1 = C.exact_inputs(node, n, NH, NW, seed=1000 * n + 31 * i + NH)
        value, _ = ref.run(node, in0, in1)
        ok, worst = C.budget_ok(ref)
        assert ok, (node, worst)
        assert np.array_equal(value.astype(np.float32).astype(np.float64), value), node
        if node == 'f18':                   # the clamp hides little: most pre-activations fall inside (0, 6)
            assert ((value > 0) & (value < 6)).mean() > 0.5


@pytest.mark.parametrize('node', N.PW_NODES)
def test_gate_rejects_a_gemm_that_lost_its_low_plane_pairs(node):
    """Resolving power: the node in float64 with both operands of every 1x1 product truncated to 16 significant bits (what three
    of the six plane pairs carry) is OUTSIDE the gate |d| <= gate_c(node) u bound at some element.  A gate that accepted it would not tell the
    split-bf16 pipe's claim from its negation."""
    h, w = ELEVEN['16x9']
    NH, NW = NET_SIZES['16x9']
    sd, layers, ref = C.checkpoint('tl')
    _, in0, in1, value, bound = _cases_16x9()[node]
    lossy, _ = N.NodeRef(layers, trunc_bits=16, bounds=False).run(node, in0, in1)
    outside = np.abs(lossy - value) > C.gate_c(node) * C.U32 * bound
    assert outside.any(), (node, float((np.abs(lossy - value) / (C.U32 * bound + 1e-300)).max()))


@functools.lru_cache(maxsize=None)
def _cases_16x9():
    h, w = ELEVEN['16x9']
    NH, NW = NET_SIZES['16x9']
    return {c[0]: c for c in C.oracle_activation_cases('tl', C.golden_frames('tl', '16x9'), h, w, NH, NW, N.PW_NODES)}


@pytest.mark.parametrize('stage', ['first', 'last'])
@pytest.mark.parametrize('bits', C.WIDE_BITS)
def test_wide_operand_exact_cases_fit_fp32_and_fill_the_planes(bits, stage):
    """The wide-operand exact cases on the CPU: every stage within 2^24 grid steps, the value an fp32 number, rows of 4 non-zeros
    that include the first and the last input channel, and operands that really span the bits they are named for."""
    xb, wb = bits
    NH, NW = NET_SIZES['16x9']
    layers = C.wide_layers(xb, wb, stage)
    span = lambda a: int(np.log2(np.abs(a[a != 0]).max() / N.grid_of(a))) + 1
    wide = [l for l in layers if l['kind'] == 'pw' and (np.abs(l['w']) > 0).sum(1).max() == 4]
    assert wide
    for l in wide:
        lo = {'us2.expand': 256, 'post_us2.expand': 128}.get(l['name'], 0)
        rows = l['w'][:l['cout']]
        assert (rows[:, lo] != 0).all() and (rows[:, -1] != 0).all() and span(rows) == wb, l['name']
    for i, node in enumerate(C.WIDE_NODES[stage]):
        ref = N.NodeRef(layers, bounds=False, track=True)
        in0, in1 = C.wide_inputs(node, 1, NH, NW, xb, seed=i)
        assert span(in0 if in1 is None else in1) == xb
        value, _ = ref.run(node, in0, in1)
        ok, worst = C.budget_ok(ref)
        assert ok, (node, worst)
        assert np.array_equal(value.astype(np.float32).astype(np.float64), value), node
        assert span(value) >= min(xb + wb, 20), (node, span(value))
