"""Pitched frames (svc_resize_frames_layout, svc_render_crops_layout) against the two things a caller could do without them:
one JSON line, and profiles/pitched_frames.json with --out.

NV12 decoder surfaces, a 32-frame batch resident in HBM: 1920 x 1080 as pitch 2048 / coded height 1088 and 3840 x 2160 as
pitch 4096 / 2176; per picture the down-scale to 140 x 250, the 9:16 window copy and 9:16 -> 1080 x 1920 (RGB out).  Legs:
  a  the layout entry on the pitched buffer
  b  a device repack into a packed tensor (two strided copies: luma, chroma), then the packed entry
  c  the packed entry on packed frames
10 warm-up launches, device events over --launches launches, the legs alternated --rounds times in one process (odd rounds
in reverse order); per leg
the values, their median and spread = (max - min) / median.  The library is driven through a few ctypes lines of its own,
so that --lib can name ANOTHER build of the packed entries (an older ABI, e.g. the parent commit's library): it then
measures leg c alone, and --merge puts that file beside this tree's numbers.  --with-lib loads such a build INTO the same
process beside this tree's library (each with a handle of its own) and alternates its packed entry, leg c_other, with the
other legs over the same buffers: that separates the two libraries from two processes' allocations.

usage: python tools/bench_layout.py [--launches 200] [--rounds 3] [--lib other.so | --with-lib other.so] [--out file.json]
                                    [--merge other.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retargetvid_amd import _lib, weights  # noqa: E402

N = 32
PICTURES = (('1920x1080_p2048_h1088', 1080, 1920, 2048, 1088, (608, 1080)),
            ('3840x2160_p4096_h2176', 2160, 3840, 4096, 2176, (1215, 2160)))
SMALL, OUT = (140, 250), (1920, 1080)            # (rows, columns)


class Lib:
    """The frame entries of a libsvc_hip.so of any ABI that has the NV12 ones."""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lib.svc_last_error.restype = ctypes.c_char_p
        lib.svc_create.argtypes = [vp, ctypes.c_size_t, i32, ctypes.POINTER(vp)]
        lib.svc_destroy.argtypes = [vp]
        lib.svc_resize_frames_nv12.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, vp]
        lib.svc_render_crops_nv12.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, vp]
        self.abi = lib.svc_abi_version()
        self.has_layout = hasattr(lib, 'svc_resize_frames_layout')
        if self.has_layout:
            lp = ctypes.POINTER(_lib.SvcFrameLayout)
            lib.svc_resize_frames_layout.argtypes = [vp, vp, lp, i32, i32, i32, vp, i32, i32, vp]
            lib.svc_render_crops_layout.argtypes = [vp, vp, lp, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, i32, vp]
        blob = weights.pack_blob(weights.fold_state_dict(weights.make_synthetic_state_dict(0)))
        self.h = vp()
        self.ok(lib.svc_create(ctypes.create_string_buffer(blob, len(blob)), len(blob), 0, ctypes.byref(self.h)))

    def ok(self, rc):
        if rc < 0:
            raise RuntimeError(self.lib.svc_last_error().decode())


def _ms(fn, launches):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def measure(L, launches, rounds, other=None):
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = {}
    for name, h, w, pitch, coded, (bw, bh) in PICTURES:
        stride = pitch * coded * 3 // 2
        pitched = torch.randint(0, 256, (N, stride), dtype=torch.uint8, device='cuda')
        luma = torch.as_strided(pitched, (N, h, w), (stride, pitch, 1))
        chroma = torch.as_strided(pitched, (N, h // 2, w), (stride, pitch, 1), pitch * coded)
        packed = torch.empty((N, h * 3 // 2, w), dtype=torch.uint8, device='cuda')
        scratch = torch.empty_like(packed)

        def repack(dst):
            dst[:, :h].copy_(luma)
            dst[:, h:].copy_(chroma)
        repack(packed)
        lay = _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), 1, stride, pitch, pitch * coded, pitch)
        rng = np.random.RandomState(0)
        x, y = rng.randint(0, w - bw + 1, N), rng.randint(0, h - bh + 1, N)
        boxes = torch.from_numpy(np.stack([x, y, x + bw, y + bh], 1).astype(np.int32)).cuda()
        for op, (oh, ow) in (('downscale_to_140x250', SMALL), ('9x16_copy', (bh, bw)), ('9x16_to_1080x1920', OUT)):
            out = torch.empty((N, oh, ow, 3), dtype=torch.uint8, device='cuda')
            if op.startswith('downscale'):
                def packed_entry(src, L=L):
                    L.ok(L.lib.svc_resize_frames_nv12(L.h, p(src), N, h, w, p(out), oh, ow, st()))

                def layout_entry():
                    L.ok(L.lib.svc_resize_frames_layout(L.h, p(pitched), ctypes.byref(lay), N, h, w, p(out), oh, ow, st()))
            else:
                def packed_entry(src, L=L):
                    L.ok(L.lib.svc_render_crops_nv12(L.h, p(src), N, h, w, p(boxes), bw, bh, p(out), oh, ow, 0, st()))

                def layout_entry():
                    L.ok(L.lib.svc_render_crops_layout(L.h, p(pitched), ctypes.byref(lay), N, h, w, p(boxes), bw, bh, p(out), 0, oh, ow, 0, st()))

            def leg_b():
                repack(scratch)
                packed_entry(scratch)
            legs = dict(c=lambda: packed_entry(packed))
            if L.has_layout:
                legs = dict(a=layout_entry, b=leg_b, c=legs['c'])
                layout_entry()
                want = out.clone()
                legs['c']()
                assert torch.equal(out, want), 'the layout entry and the packed entry disagree'
            if other is not None:
                legs['c_other'] = lambda: packed_entry(packed, other)
                out.zero_()
                legs['c_other']()
                got = out.clone()
                legs['c']()
                assert torch.equal(out, got), 'the two libraries disagree'
            ms = {k: [] for k in legs}
            for r in range(rounds):                             # odd rounds run the legs in reverse order: a leg's place in the
                order = list(legs.items())                      # sequence (what the leg before it left in the caches) shows in its values
                for k, fn in (order[::-1] if r & 1 else order):
                    ms[k].append(round(_ms(fn, launches), 4))
            row = {}
            for k, v in ms.items():
                med = float(np.median(v))
                row[k] = dict(ms_per_32=v, median=round(med, 4), spread=round((max(v) - min(v)) / med, 4))
            if L.has_layout:
                row['b_over_a'] = round(row['b']['median'] / row['a']['median'], 3)
                row['a_over_c'] = round(row['a']['median'] / row['c']['median'], 3)
            if other is not None:
                row['c_over_c_other'] = round(row['c']['median'] / row['c_other']['median'], 4)
            res['%s_%s' % (name, op)] = row
            del out
        del pitched, packed, scratch, luma, chroma
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lib', help='another build of the library: leg c only when it has no layout entries')
    ap.add_argument('--with-lib', help='another build, loaded beside this one: its packed entry is leg c_other of the same run')
    ap.add_argument('--out', help='also write the JSON to this file')
    ap.add_argument('--merge', help="a --lib run's JSON: its leg c goes beside this run's as c_other, with the ratio")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = Lib(args.lib or _lib.LIB_PATH)
    other = Lib(args.with_lib) if args.with_lib else None
    res = dict(method='NV12 surfaces, %d-frame batch resident in HBM, 10 warm-up launches, device events over %d launches, legs '
                      'alternated %d times in one process, odd rounds in reverse order; a = layout entry on the pitched buffer, b = device repack + packed '
                      'entry, c = packed entry on packed frames; spread = (max - min) / median' % (N, args.launches, args.rounds),
               abi=L.abi, library='this tree' if not args.lib else os.path.basename(os.path.dirname(os.path.abspath(args.lib))) or args.lib,
               kernels=measure(L, args.launches, args.rounds, other))
    if other is not None:
        res['other_library'] = dict(abi=other.abi, library=os.path.basename(os.path.dirname(os.path.abspath(args.with_lib))), loaded='in this process')
    if args.merge:
        other = json.load(open(args.merge))
        res['other_library'] = dict(abi=other['abi'], library=other['library'])
        for k, row in res['kernels'].items():
            row['c_other'] = other['kernels'][k]['c']
            row['c_over_c_other'] = round(row['c']['median'] / row['c_other']['median'], 3)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fp:
            json.dump(res, fp, indent=1)
            fp.write('\n')
    L.lib.svc_destroy(L.h)
    if other is not None:
        other.lib.svc_destroy(other.h)


if __name__ == '__main__':
    main()
