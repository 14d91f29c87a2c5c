"""Shared by tests/test_oracle_unisal_nodes.py, tests/test_gpu_net_nodes.py and tools/net_node_error_report.py: the shapes of the
network's nodes, the layers and inputs of the exact cases, the inputs of the full-mantissa cases, and the per-element error
ratio |device - value| / (u bound) against oracle.unisal_nodes_ref."""
import copy
import functools
import os

import numpy as np

from oracle import unisal_nodes_ref as N
from retargetvid_amd import weights

U32 = N.U32
FILL = 0xFFFFFFFF                         # svc_debug_run_node's fill: a NaN bit pattern
# nodes of the exact cases and of the per-element gate (all but 'smooth' and 'front', which have gates of their own)
MAIN_NODES = [n for n in N.NODES if n not in ('front', 'smooth')]
DEV_NODE = dict({'block%d' % i: i for i in range(2, 18)}, front=1, f18=18, skip_2x=19, skip_4x=20, post_cnn=21, us2=22, post_us2=23,
                adapt=24, smooth=25, map=26, map_profile=27, f4x=107, f2x=114)


def node_io(node, NH, NW, h, w):
    """-> (in0 shape, in1 shape or None, shape of the output buffer's row, slice of it the node owns), per frame."""
    H3, W3, H4, W4, H5, W5 = NH // 8, NW // 8, NH // 16, NW // 16, NH // 32, NW // 32
    if node.startswith('block') or node in ('f4x', 'f2x'):
        idx = {'f4x': 7, 'f2x': 14}.get(node) or int(node[5:])
        inp, oup, stride, _ = N.BLOCKS[idx]
        l = N.block_level(idx)
        d = 2 if stride == 2 and node.startswith('block') else 1
        return (NH // l, NW // l, inp), None, (NH // l // d, NW // l // d, oup), slice(0, oup)
    return {'front': ((h, w, 3), None, (NH // 2, NW // 2, 16), slice(0, 16)),
            'f18': ((H5, W5, 320), None, (H5, W5, 1296), slice(0, 1280)),
            'skip_2x': ((H4, W4, 160), None, (H4, W4, 384), slice(256, 384)),
            'skip_4x': ((H3, W3, 64), None, (H3, W3, 192), slice(128, 192)),
            'post_cnn': ((H5, W5, 1296), None, (H5, W5, 256), slice(0, 256)),
            'us2': ((H5, W5, 256), (H4, W4, 128), (H4, W4, 128), slice(0, 128)),
            'post_us2': ((H4, W4, 128), (H3, W3, 64), (H3, W3, 64), slice(0, 64)),
            'adapt': ((H3, W3, 64), None, (H3, W3), None),
            'smooth': ((H3, W3), None, (h, w), None),
            'map': ((H3, W3), None, (2, h, w), None),               # plane 0: PRE, plane 1: the uint8 map's values
            'map_profile': ((H3, W3), None, (2, h, w), None)}[node]


def run_device(eng, node, n, h, w, NH, NW, in0, in1=None):
    """The node on the device -> (the part of the output row the node owns, the rest of the row as uint32 bit patterns)."""
    _, _, oshape, own = node_io(node, NH, NW, h, w)
    row = eng.run_node(DEV_NODE[node], n, h, w, in0, in1, oshape)
    if own is None:
        return row, np.zeros(0, np.uint32)
    rest = np.ones(oshape[-1], bool)
    rest[own] = False
    return row[..., own], np.ascontiguousarray(row[..., rest]).view(np.uint32)


# ---- exact cases ----------------------------------------------------------------------------------------------------------
# Operands on dyadic grids, so that every product and every partial sum of a stage, in any order, is an fp32 number -- the
# device must then give the float64 value bit for bit.  Node inputs: multiples of 2^-3 in [-4, 4) (the low-resolution input of a
# decoder block: multiples of 2^-1, its products are blended with weights k / 16).  Weights: multiples of 2^-2, |w| <= 0.75 --
# at most 8 significant bits, so the truncating bf16 split holds them in its high plane alone.  A layer that ends in ReLU6 has 8
# non-zero weights per row (at other columns in every row) and a bias of 2 .. 4: its pre-activations then mostly fall INSIDE
# [0, 6], where the clamp hides nothing; the layers without a clamp (project, reduce, adapt) are dense.
def exact_layers(seed=11):
    rng = np.random.RandomState(seed)
    layers = copy.deepcopy(weights.fold_state_dict(weights.make_synthetic_state_dict(0)))
    nz = np.array([-0.75, -0.5, -0.25, 0.25, 0.5, 0.75])
    for l in layers:
        if l['kind'] == 'pw':
            n, k = l['w'].shape
            if l['relu6']:
                w = np.zeros((n, k))
                halves = [(0, k)] if not l['name'].endswith('us2.expand') else [(0, 2 * k // 3), (2 * k // 3, k)]     # both halves of a split expansion
                for r in range(n):
                    for lo, hi in halves:
                        w[r, lo + rng.choice(hi - lo, 8 // len(halves), replace=False)] = rng.choice(nz, 8 // len(halves))
                b = rng.randint(8, 17, n) * 0.25
            else:
                w, b = rng.randint(-3, 4, (n, k)) * 0.25, rng.randint(-8, 9, n) * 0.25
        elif l['kind'] == 'dw':
            w, b = rng.randint(-3, 4, l['w'].shape) * 0.25, rng.randint(4, 17, l['c']) * 0.25
        elif l['kind'] == 'adapt':
            w, b = rng.randint(-3, 4, 64) * 0.25, np.array([0.5])
        else:
            continue                      # stem, priors, smoothing: not in the exact cases
        l['w'], l['b'] = w.astype(np.float32), b.astype(np.float32)
    return layers


def exact_inputs(node, n, NH, NW, seed):
    """Grid inputs of `node`, every frame different."""
    rng = np.random.RandomState(seed)
    s0, s1, _, _ = node_io(node, NH, NW, 0, 0)
    if s1 is None:
        return (rng.randint(-32, 32, (n,) + s0) / 8.0).astype(np.float32), None
    return (rng.randint(-8, 8, (n,) + s0) / 2.0).astype(np.float32), (rng.randint(-32, 32, (n,) + s1) / 8.0).astype(np.float32)


def budget_ok(ref):
    """The sufficient condition of an exact case, on what a tracking NodeRef recorded: every stage spans fewer than 2^24 grid steps."""
    assert ref.budget, 'nothing tracked'
    worst = max(ref.budget, key=lambda sb: sb[1])
    return worst[1] < 2.0 ** 24, worst


# ---- exact cases with wide operands ---------------------------------------------------------------------------------------------
# The grids above give both operands a high bf16 plane only: of the six plane pairs the split pipe keeps, only h.h carries value.
# Here one 1x1 stage of every node has operands of (x, w) = (10, 10), (18, 3) and (3, 18) significant bits -- x = X 2^-xb in
# [0.5, 1) and |w| = W 2^(xb-22), X and W integers with their top bit set -- so that m.m, then m.h and l.h, then h.m and h.l carry
# value.  (18, not 20: four products of xb + wb = 21 bits span 2^23 grid steps, and a residual adds the input; more bits would
# not be fp32 numbers in every order.)  A wide row has 4 non-zeros: the first and the last input channel and two others.  The
# other stages pass values through: depthwise centre tap 1, bias 0; a 1x1 that selects one channel with weight 1.
#   stage 'first': the node's first 1x1 (expand / f18 / a skip's expansion / the skip half of a decoder expansion), weights >= 0
#                  so that its ReLU6 sees values in [0, 2); the last 1x1 selects
#   stage 'last':  the first 1x1 selects; the node's last 1x1 (project / a skip's reduction) is wide, signed
# Families with a split form: k_irb's expand (blocks 2-7, 'first'), block 7's project ('last'), k_pwr (expansions of blocks 8-17,
# decoder skip halves), k_pw_sk (f18), k_pwpw (both stages), k_dwpw's project (blocks 8-17, post_cnn, decoders, 'last').
# The low-resolution input of a decoder block is zero here: its product is blended with weights k / 16, four more bits.
WIDE_BITS = ((10, 10), (18, 3), (3, 18))
WIDE_NODES = {'first': [n for n in MAIN_NODES if n not in ('adapt', 'post_cnn')],
              'last': [n for n in MAIN_NODES if n not in ('adapt', 'f18')]}


def wide_layers(xb, wb, stage, seed=5):
    rng = np.random.RandomState(seed + 100 * xb + wb)
    layers = copy.deepcopy(weights.fold_state_dict(weights.make_synthetic_state_dict(0)))
    first = lambda name: name.endswith('.expand') or name == 'f18'
    for l in layers:
        if l['kind'] == 'dw':
            w = np.zeros(l['w'].shape)
            w[4] = 1.0
            b = np.zeros(l['c'])
        elif l['kind'] == 'pw':
            n, k = l['w'].shape
            w, b = np.zeros((n, k)), np.zeros(n)
            lo = {'us2.expand': 256, 'post_us2.expand': 128}.get(l['name'], 0)        # a decoder expansion: the skip half only
            if first(l['name']) == (stage == 'first'):
                for r in range(n):
                    cols = np.concatenate(([lo, k - 1], lo + 1 + rng.choice(k - lo - 2, 2, replace=False)))
                    W = rng.randint(2 ** (wb - 1), 2 ** wb, 4) * 2.0 ** (xb - 22)
                    w[r, cols] = W if stage == 'first' else W * rng.choice([-1.0, 1.0], 4)
            else:
                w[np.arange(n), lo + (5 * np.arange(n) + 1) % (k - lo)] = 1.0
        else:
            continue
        l['w'], l['b'] = w.astype(np.float32), b.astype(np.float32)
        assert np.array_equal(l['w'], w)
    return layers


def wide_inputs(node, n, NH, NW, xb, seed):
    rng = np.random.RandomState(seed)
    s0, s1, _, _ = node_io(node, NH, NW, 0, 0)
    one = lambda shape: (rng.randint(2 ** (xb - 1), 2 ** xb, (n,) + shape) * 2.0 ** -xb).astype(np.float32)
    if s1 is None:
        return one(s0), None
    return np.zeros((n,) + s0, np.float32), one(s1)


# ---- full-mantissa cases --------------------------------------------------------------------------------------------------
def node_inputs_from_chain(out, node):
    """The fp32-rounded inputs of `node` among the float64 activations `out` of NodeRef.chain."""
    f = lambda k: out[k].astype(np.float32)
    if node.startswith('block'):
        idx = int(node[5:])
        return f('front' if idx == 2 else 'block%d' % (idx - 1)), None
    src = {'f4x': ('block6', None), 'f2x': ('block13', None), 'f18': ('block17', None), 'skip_2x': ('f2x', None), 'skip_4x': ('f4x', None),
           'post_cnn': ('cat1', None), 'us2': ('post_cnn', 'skip_2x'), 'post_us2': ('us2', 'skip_4x'), 'adapt': ('post_us2', None),
           'smooth': ('adapt', None)}[node]
    return f(src[0]), None if src[1] is None else f(src[1])


def adversarial_seed(node, NH):
    return 1000 * MAIN_NODES.index(node) + NH


def adversarial_inputs(node, n, NH, NW, seed):
    """N(0, 1) with 1 % of the entries x100 and 10 % exact zeros."""
    rng = np.random.RandomState(seed)
    s0, s1, _, _ = node_io(node, NH, NW, 0, 0)

    def one(shape):
        x = rng.standard_normal((n,) + shape)
        x[rng.random_sample(x.shape) < 0.01] *= 100.0
        x[rng.random_sample(x.shape) < 0.10] = 0.0
        return x.astype(np.float32)
    return one(s0), None if s1 is None else one(s1)


def straddling_inputs(ref, node, n, NH, NW, seed):
    """N(0, 1) inputs moved so that pre-activations sit AT the clamps of the node's first ReLU6: at every pixel one channel of that
    stage (another at every pixel) is solved to 0 or to 6 exactly in float64; rounding the input to fp32 then leaves it a few
    u |x||w| to either side.  The stage: the expansion of a block, f18, a skip branch's expansion, a decoder's split expansion
    (solved in its skip half, on top of the up-sampled low-resolution product), post_cnn's depthwise (every third pixel each way,
    all channels, through the centre tap).  The depthwise behind an expansion is not solved for: its input is a clamped output."""
    rng = np.random.RandomState(seed)
    s0, s1, _, _ = node_io(node, NH, NW, 0, 0)
    x0 = rng.standard_normal((n,) + s0)
    x1 = None if s1 is None else rng.standard_normal((n,) + s1)
    if node == 'post_cnn':
        w, b = ref._w('post_cnn.dw')
        ok = np.abs(w[4]) > 0.05
        for it in range(2):
            pre = _dw_pre(x0, w, b)
            t = np.where(rng.random_sample(pre.shape) < 0.5, 0.0, 6.0) if it == 0 else t
            step = np.where(ok, (t - pre) / np.where(ok, w[4], 1.0), 0.0)
            x0[:, 1::3, 1::3] += step[:, 1::3, 1::3]
        return x0.astype(np.float32), None
    name = {'f18': 'f18', 'skip_2x': 'skip_2x.expand', 'skip_4x': 'skip_4x.expand', 'us2': 'us2.expand', 'post_us2': 'post_us2.expand',
            'f4x': 'f7.expand', 'f2x': 'f14.expand'}.get(node) or 'f%s.expand' % node[5:]
    w, b = ref._w(name)
    base, x = 0.0, x0
    if x1 is not None:                        # decoder: the up-sampled low-resolution product is part of the pre-activation
        Cl = s0[-1]
        base, x, w = N.up2(x0.astype(np.float32).astype(np.float64) @ w[:, :Cl].T), x1, w[:, Cl:]
    flat = x.reshape(-1, x.shape[-1])
    P = flat.shape[0]
    c = (7 * np.arange(P) + 3) % w.shape[0]
    t = np.where(rng.random_sample(P) < 0.5, 0.0, 6.0)
    pre = np.einsum('pk,pk->p', flat, w[c]) + b[c] + (base.reshape(P, -1)[np.arange(P), c] if x1 is not None else 0.0)
    flat += ((t - pre) / np.einsum('pk,pk->p', w[c], w[c]))[:, None] * w[c]
    if x1 is None:
        return flat.reshape(x0.shape).astype(np.float32), None
    return x0.astype(np.float32), flat.reshape(x1.shape).astype(np.float32)


def _dw_pre(x, w, b):
    n, H, W, C = x.shape
    xp = np.zeros((n, H + 2, W + 2, C))
    xp[:, 1:-1, 1:-1] = x
    return sum(xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W] * w[t] for t in range(9)) + b


def error_ratio(dev, value, bound):
    """max over the elements of |device - value| / (u bound); an element with bound 0 must be exact (else inf)."""
    d = np.abs(dev.astype(np.float64) - value)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, d / (U32 * bound), np.where(d > 0, np.inf, 0.0))
    return float(np.nanmax(r)) if np.isfinite(dev).all() else float('inf')


# ---- references of the full-mantissa cases ----------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ADVERSARIAL_GEOMS = ('16x9', '1x1', '2x3')          # 256x416 (13-wide lowest level), 320x320, 416x288
# The gate of the full-mantissa cases: |device - value| <= C_GATE u bound at every element, on both pipes.  Measured on the MI355X
# (profiles/net_node_error.md, written by tools/net_node_error_report.py): twice the largest ratio of the fp32 pipe over every
# node, geometry and kind.  C_SMOOTH: the same for the smoothing node.  The table's second section -- `front` and `smooth` at the map
# shapes of tests/test_net_plan_census.py on the carrier checkpoint -- enters C_NODE['front'] and C_SMOOTH by the same rule: it set
# C_NODE['front'] (2.069 at 8x8, in the carrier's pass-through channel, whose bound has few terms; tl / ri: 0.115) and left C_SMOOTH.
C_GATE = 19.226
C_SMOOTH = 194.076
# One constant for all nodes is set by the node with the fewest terms per sum; the first-order bound of a node with long sums and
# several stages overestimates its error by more, and there C_GATE alone would accept a GEMM that lost its low plane pairs
# (tests/test_oracle_unisal_nodes.py: the resolving-power test).  So each node is ALSO held to twice its own fp32 maximum of the
# same table; gate_c never exceeds C_GATE.  These constants belong to the inputs of the table: whoever changes the frames, the
# seeds or the kinds of input regenerates C_GATE, C_SMOOTH and C_NODE together with tools/net_node_error_report.py.
C_NODE = {'front': 4.138, 'block2': 0.249, 'block3': 0.533, 'block4': 0.297, 'block5': 0.485, 'block6': 0.675, 'block7': 0.441, 'block8': 0.325, 'block9': 0.468, 'block10': 0.474, 'block11': 0.226, 'block12': 0.238, 'block13': 0.365, 'block14': 0.163, 'block15': 0.240, 'block16': 0.214, 'block17': 0.174, 'f4x': 0.569, 'f2x': 0.269, 'f18': 11.793, 'skip_2x': 0.583, 'skip_4x': 0.842, 'post_cnn': 0.621, 'us2': 0.045, 'post_us2': 0.064, 'adapt': 19.226}


def gate_c(node):
    return C_SMOOTH if node == 'smooth' else min(C_GATE, C_NODE.get(node, C_GATE))


@functools.lru_cache(maxsize=None)
def checkpoint(ck):
    """(state dict, folded layers, NodeRef) of a golden checkpoint."""
    from test_oracle_unisal import golden5_checkpoint
    sd = golden5_checkpoint(ck, GOLDEN)
    layers = weights.fold_state_dict(sd)
    return sd, layers, N.NodeRef(layers, sd['smoothing_salicon.weight'])


def golden_frames(ck, gname):
    """The goldens' frames of (checkpoint, geometry), all of them."""
    from test_oracle_unisal import golden5_frames
    if gname in ('16x9', '4x3', 'port'):
        return np.load(os.path.join(GOLDEN, 'unisal_golden3.npz' if ck == 'tl' else 'unisal_golden2.npz'))['frames_' + gname]
    return golden5_frames(np.load(os.path.join(GOLDEN, 'unisal_golden5.npz')), gname)


def network_input(frames, dtype):
    """uint8 frames -> the normalised network input [n, NH, NW, 3] (oracle.unisal_ref.preprocess) as a NumPy array."""
    from oracle import unisal_ref as U
    return np.stack([U.preprocess(f, dtype=dtype).permute(1, 2, 0).numpy() for f in frames])


def gaussians(sd, NH, NW):
    import torch
    from oracle import unisal_ref as U
    g = U.gaussian_maps(torch.as_tensor(np.asarray(sd['coarse_gaussians_salicon'])), NH // 32, NW // 32, dtype=torch.float64)
    return g.permute(1, 2, 0).numpy()


def oracle_activation_cases(ck, frames, h, w, NH, NW, nodes):
    """For every node: (node, in0, in1, value, bound) on the float64 oracle's own activations rounded to fp32."""
    import torch
    sd, _, ref = checkpoint(ck)
    plain = N.NodeRef(list(ref.L.values()), ref.k41, bounds=False)
    acts = plain.chain(network_input(frames, torch.float64), (h, w), gaussians(sd, NH, NW))
    for node in nodes:
        in0, in1 = node_inputs_from_chain(acts, node)
        yield (node, in0, in1) + ref.run(node, in0, in1, out_hw=(h, w))
