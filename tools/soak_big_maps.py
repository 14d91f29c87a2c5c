#!/usr/bin/env python3
"""Maps of more than 8 192 points at every geometry the tail takes (140x250, 187x250, 250x140, 255x255: up to 65 025 points):
the round-4 kernels (k_prim_lvl_big, tp_body<2>) against the round-2 kernels (one node per step, serial union-find; verified
against the oracle) -- Prim edge list, labels, filtered maps, centres must be identical.  Covers what a 140x250 map cannot reach:
more new tree nodes than the batch table holds (> 36 864), the fourth level of the nearest-greater search, cluster tables
that overflow.  python tools/soak_big_maps.py [maps per geometry] [seed]   (GPU box)"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pipeline_ref as P
from retargetvid_amd import ops
n_maps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
old, new = ops.tail_engine(reference=True), ops.tail_engine(reference=False)
bad = 0
for (h, w) in ((140, 250), (187, 250), (250, 140), (255, 255)):
    ys, xs = np.mgrid[0:h, 0:w]
    maps = np.zeros((n_maps, h, w), np.uint8)
    for i in range(n_maps):
        kind = i % 4
        if kind == 0:
            m = 255.0 * (rng.rand(h, w) < rng.uniform(0.35, 1.0))
        elif kind == 1:
            m = np.zeros((h, w))
            for _ in range(rng.randint(1, 4)):
                cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(h / 4, h), rng.uniform(w / 4, w)
                m = np.maximum(m, 255 * np.exp(-(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)))
        elif kind == 2:
            m = 255.0 * (np.sin(xs / rng.uniform(2, 9)) * np.sin(ys / rng.uniform(2, 9)) > rng.uniform(-0.8, 0.0))
        else:
            m = np.full((h, w), 255.0)
            m[rng.rand(h, w) < rng.uniform(0.0, 0.2)] = 0
        u = np.clip(m + rng.uniform(0, 30) * rng.rand(h, w), 0, 255).astype(np.uint8)
        u[u < 120] = 0
        maps[i] = u
    flags = (rng.rand(n_maps) < 0.25).astype(np.uint8); flags[-1] = 0
    for CP in (P.init_crop_params(), dict(P.init_crop_params(), hdbscan_min=40, hdbscan_min_samples=5, select_sum=1)):
        a, b = torch.from_numpy(maps).cuda(), torch.from_numpy(maps).cuda()
        xa, sa = old.cluster_center_(a, flags, CP, want_stats=True)
        xb, sb = new.cluster_center_(b, flags, CP, want_stats=True)
        ok = torch.equal(a, b) and torch.equal(sa, sb) and np.array_equal(xa.cpu().numpy(), xb.cpu().numpy(), equal_nan=True)
        detail = []
        for i in range(n_maps):
            s_old, s_new = old.cluster_state(i, h * w), new.cluster_state(i, h * w)
            same = np.array_equal(s_old['mst'], s_new['mst']) and np.array_equal(s_old['labels'], s_new['labels'])
            ok = ok and same
            detail.append('%d%s%s' % (s_new['n'], '' if same else '!', '' if s_new['hdr'][ops.HDR_TREE_PAR] else 's'))
        bad += 0 if ok else 1
        print('%3dx%3d mcs %2d: %s   points per map (! = differs, s = hierarchy by the serial builder): %s' % (h, w, CP['hdbscan_min'], 'identical' if ok else 'MISMATCH', ' '.join(detail)), flush=True)
print('mismatching (geometry, parameter set) pairs:', bad)
sys.exit(1 if bad else 0)
