"""-m gpu: k_pwr's staged operands, piece by piece (svc_debug_run_node against oracle/unisal_nodes_ref.py, both matrix pipes).

k_pwr brings its weight chunk to LDS as 16-byte pieces, up to 15 per thread, all requested before the first is waited for.  The
exact cases of tests/test_gpu_net_nodes.py put 8 non-zeros in a weight row, or 4 wide ones, and would pass with a piece of the
middle or low bf16 plane dropped or one slot off.  Here the staged weights are DENSE, 18 significant bits each, in [2^-3, 2^-2), built so that all three planes of the copies' round-to-nearest split are live
at every element (asserted on a host restatement of the split; with 17 bits the low plane of that split is always zero), and
the activations are SPARSE one-bit values (0.5 or 1.0) on 16 channels per pixel -- other channels at every pixel, all of
them covered -- so that every partial sum, in any order, is an fp32 number (budget_ok on a tracking NodeRef) and the device must
equal the float64 value bit for bit.  The other stages pass values through as in net_node_cases.wide_layers; the project, which
selects as many expanded channels as the node has outputs, is rotated over six cases until every expanded channel has reached
the output.  Two scratch builds fail it at the first case: the last piece of a thread's batch not stored (4 576 of 26 624
elements differ), one row of the chunk stored one piece further on (415 differ): profiles/pwr_staging_resources.txt.

Nodes: block8 (K = 64), block12 (96), block15 (160), us2 (K = 128 with the up-sampled term), post_us2 (K = 128 without, K = 64
with).  Shapes: 256x416 at n = 1 -- M = 104 at level 5 (a single partial row block), 416 at level 4 --, 320x320 at n = 1 (M =
1 600 at level 3, 400, 100), 256x416 at n = 3.  A decoder block runs twice: its low-resolution input zero and 16 non-zeros per
skip pixel, and both inputs live with 1 + 2 non-zeros (the 2x bilinear blend multiplies by k / 16: four more bits).

The last stage, k_smooth_down_mfma (SVC_NODE_SMOOTH): PRE on random logits at 140x250, at a strip where the plan gives fewer
than seven rows per band, and at the smallest map of the census must equal, bit for bit, the PRE of an engine planned with one
row per band (SVC_SD_ROWS=1) -- the first and the last band are among the rows compared."""
import os

import numpy as np
import pytest

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import net_node_cases as C
from oracle import unisal_nodes_ref as N
from retargetvid_amd import ops
from test_oracle_unisal import ELEVEN, NET_SIZES

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

PIPES = ('bf16x6', 'f32')
NODES = ('block8', 'block12', 'block15', 'us2', 'post_us2')
SHAPES = (('16x9', 1), ('1x1', 1), ('16x9', 3))
# Non-zeros per pixel.  A product is an 18-bit weight below 2^-2 times 0.5 or 1.0: a multiple of 2^-21; 16 of them stay below 4, a
# block's residual adds an input of at most 1: below 5 x 2^21 steps, inside the 2^24 of an fp32 number whatever the order (32
# non-zeros would leave it).  With both inputs of a decoder block live the blend's k / 16 makes the grid 2^-24 (values 1.0 only):
# 1 + 2 non-zeros stay below 3 x 2^-2 = 0.75 x 2^24 steps.
NNZ = 16
ROTATIONS = 6           # expanded channels / outputs of every node above: 384 / 64, 576 / 96, 960 / 160, 768 / 128, 384 / 64


def _engine(pipe, layers, env=()):
    old = {k: os.environ.get(k) for k in ('SVC_MX',) + tuple(k for k, _ in env)}
    os.environ['SVC_MX'] = pipe
    os.environ.update(dict(env))
    try:
        eng = ops.Engine() if layers is None else ops.Engine.from_layers(layers)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert eng.matrix_pipe() == pipe
    return eng


def dense_layers(rot, seed=3):
    """wide_layers' pass-through network with DENSE 18-bit first 1x1 stages; the selecting 1x1 of a node with n outputs takes
    expanded channels rot n .. rot n + n - 1."""
    rng = np.random.RandomState(seed)
    layers = C.wide_layers(10, 10, 'first')
    for l in layers:
        if l['kind'] != 'pw':
            continue
        n, k = l['w'].shape
        if l['name'].endswith('.expand'):
            # W = 1024 H + R, 129 <= H < 256, R odd, 256 < |R| < 512: 18 significant bits, and the round-to-nearest split of the
            # weight copies gives h = 1024 H, m = R to eight bits, l = +-1 -- all three planes live at EVERY element
            R = (2 * rng.randint(128, 256, (n, k)) + 1) * rng.choice([-1, 1], (n, k))
            w = (1024 * rng.randint(129, 256, (n, k)) + R) * 2.0 ** -20                # in [2^-3, 2^-2)
        else:
            w = np.zeros((n, k))
            w[np.arange(n), (rot * n + np.arange(n)) % k] = 1.0
        l['w'] = w.astype(np.float32)
        assert np.array_equal(l['w'], w)
    return layers


def _bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _every_piece_of_every_plane_is_live(w):
    """The three round-to-nearest bf16 planes of a weight matrix: every group of 8 consecutive k of every row non-zero."""
    h = _bf16_rne(w)
    m = _bf16_rne(w - h)
    lo = _bf16_rne(w - h - m)
    return all((p.reshape(w.shape[0], -1, 8) != 0).any(axis=2).all() for p in (h, m, lo))


def sparse(rng, shape, nnz, values=(0.5, 1.0)):
    """One-bit values on nnz channels of every pixel, other channels at every pixel: random ones, or, where nnz is too small for
    chance to cover the channels, pixel p takes channels p nnz .. p nnz + nnz - 1 (mod k)."""
    k = shape[-1]
    flat = np.zeros((int(np.prod(shape[:-1])), k), np.float32)
    for p in range(flat.shape[0]):
        flat[p, rng.choice(k, nnz, replace=False) if nnz >= 8 else (p * nnz + np.arange(nnz)) % k] = rng.choice(values, nnz)
    assert (flat != 0).any(axis=0).all() or flat.shape[0] * nnz < k, 'an input channel no pixel carries'
    return flat.reshape(shape)


def pwr_inputs(node, n, NH, NW, mix, seed):
    rng = np.random.RandomState(seed)
    s0, s1, _, _ = C.node_io(node, NH, NW, 0, 0)
    if s1 is None:
        return sparse(rng, (n,) + s0, NNZ), None
    if mix == 'skip':
        return np.zeros((n,) + s0, np.float32), sparse(rng, (n,) + s1, NNZ)
    return sparse(rng, (n,) + s0, 1, (1.0,)), sparse(rng, (n,) + s1, 2, (1.0,))


def test_the_dense_weights_fill_every_piece_of_every_plane():
    layers = dense_layers(0)
    seen = 0
    for l in layers:
        if l['kind'] == 'pw' and l['name'].endswith('.expand') and l['name'].split('.')[0] in ('f8', 'f12', 'f15', 'us2', 'post_us2'):
            assert _every_piece_of_every_plane_is_live(l['w']), l['name']
            seen += 1
    assert seen == 5


@pytest.mark.parametrize('rot', range(ROTATIONS))
def test_dense_weight_chunks_reach_the_tiles_piece_by_piece(rot):
    layers = dense_layers(rot)
    engs = {pipe: _engine(pipe, layers) for pipe in PIPES}
    try:
        for gname, n in SHAPES:
            h, w = ELEVEN[gname]
            NH, NW = NET_SIZES[gname]
            for i, node in enumerate(NODES):
                for mix in (('skip', 'both') if node in ('us2', 'post_us2') else ('one',)):
                    ref = N.NodeRef(layers, bounds=False, track=True)
                    in0, in1 = pwr_inputs(node, n, NH, NW, mix, seed=1000 * rot + 77 * i + NH + n)
                    value, _ = ref.run(node, in0, in1)
                    ok, worst = C.budget_ok(ref)
                    assert ok, (node, mix, 'a partial sum may not be an fp32 number', worst)
                    assert (value != 0).any(), (node, mix, 'nothing reached the output')
                    for pipe in PIPES:
                        where = (rot, gname, n, node, mix, pipe)
                        dev, rest = C.run_device(engs[pipe], node, n, h, w, NH, NW, in0, in1)
                        assert not np.isnan(dev).any(), (where, 'unwritten elements', int(np.isnan(dev).sum()))
                        bad = dev.astype(np.float64) != value
                        assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(dev - value).max()))
                        assert (rest == C.FILL).all(), (where, 'the part of the row the node does not own was written')
    finally:
        for e in engs.values():
            e.close()


# ---- the last stage -----------------------------------------------------------------------------------------------------------------
# (h, w): the headline map; a strip whose plan gives fewer than seven rows per band; the smallest map of the census
SMOOTH_SHAPES = ((140, 250), (27, 250), (8, 8))


@pytest.mark.parametrize('hw', SMOOTH_SHAPES)
def test_smoothing_equals_the_one_row_per_band_engine_bit_for_bit(hw):
    h, w = hw
    plan = ops.net_plan(h, w)
    NH, NW = plan['NH'], plan['NW']
    if hw == (27, 250):
        assert 1 < plan['sd_rows'] < 7, plan
    rng = np.random.RandomState(h * 1000 + w)
    logits = rng.standard_normal((2, NH // 8, NW // 8)).astype(np.float32) * 4.0
    out = {}
    for rows in (0, 1):
        eng = _engine('bf16x6', None, env=(('SVC_SD_ROWS', str(rows)),) if rows else ())
        try:
            out[rows] = eng.run_node(C.DEV_NODE['smooth'], 2, h, w, logits, None, (h, w))
        finally:
            eng.close()
    assert not np.isnan(out[0]).any() and not np.isnan(out[1]).any()
    a, b = out[0].view(np.uint32), out[1].view(np.uint32)
    for rows in (slice(0, plan['sd_rows']), slice(h - plan['sd_rows'], h), slice(0, h)):      # first band, last band, everything
        assert np.array_equal(a[:, rows], b[:, rows]), (hw, rows, int((a[:, rows] != b[:, rows]).sum()))
