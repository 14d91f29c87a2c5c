"""One leg of the NV12 colour A/B (profiles/nv12_colour.json): the NV12 rows of tools/bench_render.py (copy, INTER_LINEAR, the
--lanczos shape; to RGB and to NV12) and the NV12 down-scale rows of tools/bench_layout.py (packed and pitched), on the library
SVC_LIB names (or the tree's own), at one colour; 32 resident frames, ms per launch from device events, ROUNDS values per row.

usage: [SVC_LIB=<another build's libsvc_hip.so>] python tools/bench_nv12_colour.py TAG default|bt709full OUT.json

A build without the colour entries (the parent commit's) loads under this binding and serves the `default` legs.  For an A/B run
the legs in processes of their own, alternating the two libraries, and compare a build against the spread of the other's legs."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from retargetvid_amd import _lib, ops  # noqa: E402

tag, colour, out_fn = sys.argv[1:4]
col = None if colour == 'default' else ('bt709', 'full')
LAUNCHES, ROUNDS, N = 100, 3, 32


def event_ms(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / LAUNCHES, 4)


def boxes_for(n, h, w, bw, bh, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, w - bw + 1, n)
    y = rng.randint(0, h - bh + 1, n)
    return np.stack([x, y, x + bw, y + bh], 1).astype(np.int32)


RENDER = (('640x360_1x3_copy', (360, 640), (120, 360), None, 'linear'),
          ('1920x1080_9x16_copy', (1080, 1920), (608, 1080), None, 'linear'),
          ('1920x1080_9x16_to_1080x1920', (1080, 1920), (608, 1080), (1080, 1920), 'linear'),
          ('3840x2160_9x16_to_1080x1920', (2160, 3840), (1215, 2160), (1080, 1920), 'linear'),
          ('4k_1215x2160_to_720x1280_lanczos', (2160, 3840), (1215, 2160), (720, 1280), 'lanczos'))
DOWN = (('1920x1080', 1080, 1920, 2048, 1088), ('3840x2160', 2160, 3840, 4096, 2176))

eng = ops.Engine()
rows = {}
for name, (h, w), (bw, bh), osz, interp in RENDER:
    ow, oh = osz or (bw, bh)
    frames = torch.randint(0, 256, (N, h * 3 // 2, w), dtype=torch.uint8, device=eng.device)
    boxes = torch.from_numpy(boxes_for(N, h, w, bw, bh)).to(eng.device)
    for f in ('rgb24', 'nv12'):
        dst = torch.empty((N,) + ops.frame_shape(f, oh, ow), dtype=torch.uint8, device=eng.device)
        kw = {}
        if col is not None:
            kw = dict(colour=col, out_colour=col if f == 'nv12' else None)
        fn = lambda: eng._render(frames, boxes, bw, bh, dst, False, 'nv12', f, None, interp, **kw)
        rows['render_%s_to_%s' % (name, f)] = [event_ms(fn) for _ in range(ROUNDS)]
        del dst
    del frames
    torch.cuda.empty_cache()
for name, h, w, pitch, coded_h in DOWN:
    packed = torch.randint(0, 256, (N, h * 3 // 2, w), dtype=torch.uint8, device=eng.device)
    kw = {} if col is None else dict(colour=col)
    rows['downscale_%s_packed' % name] = [event_ms(lambda: eng.resize_frames(packed, 140, 250, 'nv12', **kw)) for _ in range(ROUNDS)]
    del packed
    L = ops.frame_layout('nv12', h, w, dict(pitch=pitch, chroma_offset=pitch * coded_h), pitch * coded_h * 3 // 2)
    pitched = torch.randint(0, 256, (N, L.frame_stride), dtype=torch.uint8, device=eng.device)
    rows['downscale_%s_pitch%d' % (name, pitch)] = [event_ms(lambda: eng.resize_frames(pitched, 140, 250, 'nv12', L, **kw)) for _ in range(ROUNDS)]
    del pitched
    torch.cuda.empty_cache()
eng.close()
res = dict(tag=tag, colour=colour, lib=_lib.LIB_PATH, launches=LAUNCHES, rounds=ROUNDS, frames=N, ms_per_32=rows)
os.makedirs(os.path.dirname(os.path.abspath(out_fn)), exist_ok=True)
with open(out_fn, 'w') as fp:
    json.dump(res, fp, indent=1)
print(tag, colour, {k: float(np.median(v)) for k, v in rows.items()})
