"""Oracle: the saliency network NODE BY NODE in float64, each with a running error bound.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Evaluates one node of the graph that csrc/svc_net.hip walks
(forward_chunk: front, cnn.features.2 .. 17, features.18, the two skip branches, post_cnn, the two decoder blocks,
adaptation, smoothing) from the FOLDED layers (retargetvid_amd.weights.fold_state_dict: the fp32 numbers the device
holds, cast to float64) on NHWC arrays [n, H, W, C].  No BatchNorm modules, no torch convolutions: every operation is
restated here in NumPy -- 1x1 (pw), depthwise 3x3 stride 1 or 2 with pad 1, ReLU6, residual, ::2, bilinear x2
(align_corners=False), the decoder's split expansion, the adaptation -- except the smoothing, which is the graph's own
formulation (nearest x8, replicate pad 20, the checkpoint's 41x41 kernel, bilinear to the map size) on torch's float64
resampling.  tests/test_oracle_unisal_nodes.py pins the chain of all nodes against oracle.unisal_ref.forward_logits.

Every node returns (value, bound).  `bound` is a first-order running error bound in units of u = 2^-24 for an fp32
evaluation of the node IN ANY ORDER: each stage adds its own sum of absolute terms, sum|x||w| + |b|, to the bound of
its input pushed through |w| -- the same evaluator run on absolute values.  ReLU6 and ::2 pass the bound through
(clamping is 1-Lipschitz and exact), the node's input is exact (bound 0).  |device - value| <= C u bound with a small C
is then a per-ELEMENT gate: an element that is small because large terms cancel is allowed their rounding, an element
that is small because its terms are small is not allowed the tensor's maximum.

trunc_bits=16 evaluates every 1x1 product with both operands truncated to that many significant bits: the arithmetic of
a split-bf16 GEMM that lost its low plane pairs.  A gate that accepts its result resolves nothing."""
import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32

BLOCKS = {}               # idx -> (inp, oup, stride, expand) of cnn.features.idx


def _init_blocks():
    stages = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1)]
    inp, idx = 32, 1
    for t, c, n, s in stages:
        for i in range(n):
            BLOCKS[idx] = (inp, c, s if i == 0 else 1, t)
            inp = c
            idx += 1


_init_blocks()

# node name -> (inputs, output): per-frame (divisor of the network size, channels); None = special
NODES = ['front'] + ['block%d' % i for i in range(2, 18)] + ['f4x', 'f2x', 'f18', 'skip_2x', 'skip_4x', 'post_cnn', 'us2',
                                                               'post_us2', 'adapt', 'smooth']
PW_NODES = [n for n in NODES if n not in ('front', 'adapt', 'smooth')]        # the nodes whose 1x1 layers run on the matrix pipe


def block_level(idx):
    """Divisor of the network size at the INPUT of cnn.features.idx (2 at block 2)."""
    d = 2
    for i in range(2, idx):
        if BLOCKS[i][2] == 2:
            d *= 2
    return d


def trunc_sig(a, bits):
    """a with its significand truncated (towards zero) to `bits` significant bits."""
    m, e = np.frexp(a)
    return np.ldexp(np.trunc(m * 2.0 ** bits) * 2.0 ** -bits, e)


def grid_of(a):
    """The largest power of two that divides every entry of a (1.0 for an all-zero array)."""
    a = np.asarray(a, np.float64)
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    M = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = np.log2((M & -M).astype(np.float64)).astype(np.int64)        # position of the lowest set bit of the significand
    return 2.0 ** int((e.astype(np.int64) - 53 + low).min())


def relu6(v):
    return np.clip(v, 0.0, 6.0)


def up2(x):
    """Bilinear x2, align_corners=False, on axes 1 and 2 of [n, H, W, C]: weights 0.75 / 0.25, the border replicated."""
    for ax in (1, 2):
        n = x.shape[ax]
        i = np.arange(n)
        lo, hi = np.take(x, np.maximum(i - 1, 0), ax), np.take(x, np.minimum(i + 1, n - 1), ax)
        even, odd = 0.25 * lo + 0.75 * x, 0.75 * x + 0.25 * hi
        shape = list(x.shape)
        shape[ax] = 2 * n
        x = np.stack((even, odd), axis=ax + 1).reshape(shape)
    return x


class NodeRef:
    """The nodes of one checkpoint.  layers: weights.fold_state_dict(sd); k41: the checkpoint's 41x41 smoothing kernel
    (smoothing_salicon.weight), needed by 'smooth' only."""

    def __init__(self, layers, k41=None, trunc_bits=None, bounds=True, track=False):
        self.L = {l['name']: l for l in layers}
        self.k41 = None if k41 is None else np.asarray(k41, np.float64).reshape(41, 41)
        self.trunc_bits = trunc_bits
        self.bounds = bounds          # False: values only (the bound comes back as 0)
        self.track = track            # True: self.budget collects (stage, max sum of |terms| / grid of the terms) -- see budget
        self.budget = []

    def _spend(self, stage, sum_abs, *grids):
        """Records how many grid steps the largest sum of absolute terms of a stage spans.  Below 2^24, every partial sum of the
        stage, in any order, is an fp32 number: it is a multiple of the grid (the product of the operands' grids) no larger than
        2^24 grid steps."""
        g = np.prod([float(v) for v in grids])
        self.budget.append((stage, float(np.max(sum_abs)) / g))

    # ---- stages: (value, bound) -> (value, bound) -------------------------------------------------------
    def _w(self, name, cols=None):
        l = self.L[name]
        w = l['w'].astype(np.float64)
        if cols is not None:
            w = w[:, cols]
        return w, l['b'].astype(np.float64)

    def pw(self, x, e, w, b, act):
        """x [.., K] . w[N, K]^T + b; b None: no bias (the low-resolution half of a split expansion)."""
        xa, wa = np.abs(x), np.abs(w)
        if self.trunc_bits:
            x, w = trunc_sig(x, self.trunc_bits), trunc_sig(w, self.trunc_bits)
        v = x @ w.T
        eo = (xa + e) @ wa.T if self.bounds else 0.0
        if b is not None:
            v = v + b
            eo = eo + np.abs(b)
        if self.track:
            g = grid_of(x) * grid_of(w)
            assert b is None or grid_of(b) >= g
            self._spend('pw %dx%d' % w.shape, xa @ wa.T + (0.0 if b is None else np.abs(b)), g)
        if not self.bounds:
            eo = 0.0
        return (relu6(v), eo) if act else (v, eo)

    def dw(self, x, e, name, stride):
        """Depthwise 3x3, pad 1, + bias, ReLU6; weights [9][C], tap = 3 ky + kx.  stride 2 = stride 1 then ::2."""
        w, b = self._w(name)
        n, H, W, C = x.shape
        xp = np.zeros((n, H + 2, W + 2, C))
        ap = np.zeros((n, H + 2, W + 2, C))
        xp[:, 1:-1, 1:-1], ap[:, 1:-1, 1:-1] = x, np.abs(x) + e
        v, eo = np.zeros_like(x) + b, np.zeros_like(x) + np.abs(b)
        for t in range(9):
            ky, kx = divmod(t, 3)
            v += xp[:, ky:ky + H, kx:kx + W] * w[t]
            if self.bounds or self.track:
                eo += ap[:, ky:ky + H, kx:kx + W] * np.abs(w[t])
        if self.track:                                  # (tracking runs on exact inputs: e = 0, eo = the sum of absolute terms)
            g = grid_of(x) * grid_of(w)
            assert grid_of(b) >= g
            self._spend('dw %d' % C, eo, g)
        v = relu6(v)
        if stride == 2:
            v, eo = v[:, ::2, ::2], eo[:, ::2, ::2]
        return v, (eo if self.bounds else 0.0)

    def inv_res(self, x, e, name, stride, expand, residual):
        y, ey = x, e
        if expand:
            y, ey = self.pw(y, ey, *self._w(name + '.expand'), True)
        y, ey = self.dw(y, ey, name + '.dw', stride)
        y, ey = self.pw(y, ey, *self._w(name + '.project'), False)
        if residual:
            if self.track:
                self._spend('residual', np.abs(x) + np.abs(y), min(grid_of(x), grid_of(y)))
            y, ey = x + y, (e + ey + np.abs(x) + np.abs(y) if self.bounds else 0.0)
        return y, ey

    def decoder(self, lo, skip, name):
        """expand(concat(up(lo), skip)) as the device splits it: relu6(up(W[:, :Cl] . lo) + W[:, Cl:] . skip + b), then depthwise
        and project."""
        Cl = lo.shape[-1]
        w, b = self._w(name + '.expand')
        t, et = self.pw(lo, 0.0, w[:, :Cl], None, False)
        u, eu = up2(t), (up2(et) + up2(np.abs(t)) if self.bounds else 0.0)
        s, es = self.pw(skip, 0.0, w[:, Cl:], b, False)
        if self.track:                                  # the blend (weights 9/16, 3/16, 1/16 of four taps) and the sum of the two halves
            self._spend('up2 + skip half', up2(np.abs(t)) + np.abs(s), min(grid_of(t) / 16, grid_of(s)))
        v, ev = relu6(u + s), (eu + es + np.abs(u) + np.abs(s) if self.bounds else 0.0)
        v, ev = self.dw(v, ev, name + '.dw', 1)
        return self.pw(v, ev, *self._w(name + '.project'), False)

    def stem(self, x):
        """3x3 stride 2 pad 1, 3 -> 32, + bias, ReLU6; weights [ky][kx][cin][cout]."""
        l = self.L['stem']
        w, b = l['w'].astype(np.float64).reshape(3, 3, 3, 32), l['b'].astype(np.float64)
        n, H, W, _ = x.shape
        xp = np.zeros((n, H + 2, W + 2, 3))
        xp[:, 1:-1, 1:-1] = x
        v, e = np.zeros((n, H // 2, W // 2, 32)) + b, np.zeros((n, H // 2, W // 2, 32)) + np.abs(b)
        for ky in range(3):
            for kx in range(3):
                p = xp[:, ky:ky + H:2, kx:kx + W:2]
                v += p @ w[ky, kx]
                e += np.abs(p) @ np.abs(w[ky, kx])
        return relu6(v), e

    def smooth(self, logit, out_hw):
        """[n, H3, W3] -> [n, h, w]: nearest x8, replicate pad 20, 41x41 convolution, bilinear (align_corners=False)."""
        import torch
        import torch.nn.functional as F

        def run(a, k):
            y = F.interpolate(torch.from_numpy(a)[:, None], scale_factor=8, mode='nearest')
            y = F.conv2d(F.pad(y, [20] * 4, mode='replicate'), torch.from_numpy(k)[None, None])
            return y, F.interpolate(y, size=tuple(out_hw), mode='bilinear', align_corners=False)[:, 0].numpy()

        y, v = run(np.ascontiguousarray(logit, np.float64), self.k41)
        if not self.bounds:                                              # the value alone: half the convolutions
            return v, 0.0
        _, e1 = run(np.abs(logit), np.abs(self.k41))                      # the convolution's terms through the blend
        e2 = F.interpolate(y.abs(), size=tuple(out_hw), mode='bilinear', align_corners=False)[:, 0].numpy()   # the blend's own
        return v, e1 + e2

    # ---- nodes -----------------------------------------------------------------------------------------
    def run(self, node, in0, in1=None, out_hw=None):
        """(value, bound) of `node` on float64-castable NHWC input(s).  'front': in0 = the normalised network input
        [n, NH, NW, 3].  'f4x' / 'f2x': cnn.features.7 / 14 at full resolution ('block7' / 'block14': behind ::2).  'f18',
        'skip_2x', 'skip_4x': the node's own channels (1280 / 128 / 64).  'adapt' -> [n, H3, W3]; 'smooth' takes that and
        out_hw = (h, w)."""
        x = np.asarray(in0, np.float64)
        if node == 'front':
            v, e = self.stem(x)
            return self.inv_res(v, e, 'f1', 1, False, False)
        if node.startswith('block') or node in ('f4x', 'f2x'):
            idx = {'f4x': 7, 'f2x': 14}.get(node) or int(node[5:])
            inp, oup, stride, t = BLOCKS[idx]
            tap = idx in (7, 14)
            v, e = self.inv_res(x, 0.0, 'f%d' % idx, 1 if tap else stride, True, stride == 1 and inp == oup)
            if tap and node.startswith('block'):
                v, e = v[:, ::2, ::2], (e[:, ::2, ::2] if self.bounds else 0.0)
            return v, e
        if node == 'f18':
            return self.pw(x, 0.0, *self._w('f18'), True)
        if node in ('skip_2x', 'skip_4x'):
            v, e = self.pw(x, 0.0, *self._w(node + '.expand'), True)
            return self.pw(v, e, *self._w(node + '.reduce'), False)
        if node == 'post_cnn':
            return self.inv_res(x, 0.0, 'post_cnn', 1, False, False)
        if node in ('us2', 'post_us2'):
            return self.decoder(x, np.asarray(in1, np.float64), node)
        if node == 'adapt':
            l = self.L['adapt']
            w, b = l['w'].astype(np.float64), float(l['b'][0])
            if self.track:
                self._spend('adapt', np.abs(x) @ np.abs(w) + abs(b), grid_of(x) * grid_of(w))
            return x @ w + b, np.abs(x) @ np.abs(w) + abs(b)
        if node == 'smooth':
            return self.smooth(x, out_hw)
        raise KeyError(node)

    def chain(self, x, out_hw, gauss):
        """Every node in turn from the network input x [n, NH, NW, 3]; gauss [H5, W5, 16]: the prior maps.  -> {node: value},
        plus 'cat1' (the 1296-channel row post_cnn reads)."""
        out = {}
        v = out['front'] = self.run('front', x)[0]
        for idx in range(2, 18):
            if idx in (7, 14):
                out['f4x' if idx == 7 else 'f2x'] = self.run('f4x' if idx == 7 else 'f2x', v)[0]
            v = out['block%d' % idx] = self.run('block%d' % idx, v)[0]
        out['f18'] = self.run('f18', v)[0]
        out['skip_2x'] = self.run('skip_2x', out['f2x'])[0]
        out['skip_4x'] = self.run('skip_4x', out['f4x'])[0]
        out['cat1'] = np.concatenate((out['f18'], np.broadcast_to(gauss, out['f18'].shape[:3] + (16,))), axis=3)
        out['post_cnn'] = self.run('post_cnn', out['cat1'])[0]
        out['us2'] = self.run('us2', out['post_cnn'], out['skip_2x'])[0]
        out['post_us2'] = self.run('post_us2', out['us2'], out['skip_4x'])[0]
        out['adapt'] = self.run('adapt', out['post_us2'])[0]
        out['smooth'] = self.run('smooth', out['adapt'], out_hw=out_hw)[0]
        return out


def state_dict_from_layers(layers, sd):
    """A state dict in the reference's key layout whose convolutions hold the FOLDED weights (float64) and whose BatchNorms are
    identities carrying the folded bias: what oracle.unisal_ref evaluates to compare graphs on the same numbers.  Gaussians,
    adaptation and smoothing come from `sd`."""
    L = {l['name']: l for l in layers}
    out = {k: np.asarray(sd[k]) for k in ('coarse_gaussians_salicon', 'adaptation_salicon.0.weight', 'adaptation_salicon.0.bias',
                                          'smoothing_salicon.weight')}

    def put(conv, bn, l):
        w = l['w'].astype(np.float64)
        if l['kind'] == 'stem':
            w = w.reshape(3, 3, 3, 32).transpose(3, 2, 0, 1)
        elif l['kind'] == 'dw':
            w = w.T.reshape(-1, 1, 3, 3)
        else:
            w = w.reshape(l['cout'], l['cin'], 1, 1)
        c = w.shape[0]
        out[conv + '.weight'] = np.ascontiguousarray(w)
        out[bn + '.weight'], out[bn + '.bias'] = np.ones(c), l['b'].astype(np.float64)
        out[bn + '.running_mean'], out[bn + '.running_var'] = np.zeros(c), np.full(c, 1.0 - 1e-5)     # + eps = 1

    def inv_res(prefix, name, expand):
        if expand:
            put(prefix + '.0', prefix + '.1', L[name + '.expand'])
            put(prefix + '.3', prefix + '.4', L[name + '.dw'])
            put(prefix + '.6', prefix + '.7', L[name + '.project'])
        else:
            put(prefix + '.0', prefix + '.1', L[name + '.dw'])
            put(prefix + '.3', prefix + '.4', L[name + '.project'])

    put('cnn.features.0.0', 'cnn.features.0.1', L['stem'])
    for idx in range(1, 18):
        inv_res('cnn.features.%d.conv' % idx, 'f%d' % idx, BLOCKS[idx][3] != 1)
    put('cnn.features.18.0', 'cnn.features.18.1', L['f18'])
    for name in ('skip_2x', 'skip_4x'):
        put(name + '.expansion.0', name + '.expansion.1', L[name + '.expand'])
        put(name + '.reduction.0', name + '.reduction.1', L[name + '.reduce'])
        out[name + '.reduction.0.bias'] = np.zeros(L[name + '.reduce']['cout'])
    inv_res('post_cnn.inv_res.conv', 'post_cnn', False)
    inv_res('upsampling_2.inv_res.conv', 'us2', True)
    inv_res('post_upsampling_2.inv_res.conv', 'post_us2', True)
    return out
