"""Pitched output (svc_render_crops_to_layout) against what a caller had to do without it -- render packed, then repack every
output byte into the encoder's surface: one JSON line, and profiles/pitched_output.json with --out.

NV12 decoder surfaces, a 32-frame batch resident in HBM: 1920 x 1080 as pitch 2048 / coded height 1088 and 3840 x 2160 as
pitch 4096 / 2176, read where they lie by every leg.  Per picture the 9:16 window copy (608 x 1080; 1216 x 2160, even for the
NV12 sink) and that window resampled to 1080 x 1920, INTER_LINEAR and Lanczos; each to NV12 and to RGB.  The output layout is this
bench's own choice, not a claim about a particular encoder: pitch = the row's bytes rounded up to 256 (the width for NV12), the
chroma plane behind the height rounded up to 16, frames pitch * coded height (* 3 / 2) apart.  Legs:
  a        the new entry into the pitched buffer
  b        svc_render_crops_colour into a packed tensor, then a device repack into the same pitched buffer (one strided copy per plane)
  c        svc_render_crops_colour alone (the packed output)
  c_other  the packed entry of ANOTHER build (--with-lib, e.g. the parent commit's library) loaded into the same process with a handle
           of its own, over the same buffers
10 warm-up launches, device events over --launches launches, the legs alternated --rounds times in one process (odd rounds in
reverse order); per leg the values, their median and spread = (max - min) / median.  Before timing, the picture bytes leg a wrote
are compared with leg c's.

usage: python tools/bench_out_layout.py [--launches 100] [--rounds 3] [--with-lib other.so] [--out file.json]"""
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
            ('3840x2160_p4096_h2176', 2160, 3840, 4096, 2176, (1216, 2160)))
OUT = (1920, 1080)               # (rows, columns)
NV12, RGB = 1, 0


class Lib:
    """The render entries of a libsvc_hip.so that has svc_render_crops_colour (and, this tree's, svc_render_crops_to_layout)."""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lp, cp = ctypes.POINTER(_lib.SvcFrameLayout), ctypes.POINTER(_lib.SvcColour)
        lib.svc_last_error.restype = ctypes.c_char_p
        lib.svc_create.argtypes = [vp, ctypes.c_size_t, i32, ctypes.POINTER(vp)]
        lib.svc_destroy.argtypes = [vp]
        lib.svc_render_crops_colour.argtypes = [vp, vp, lp, cp, i32, i32, i32, vp, i32, i32, vp, i32, cp, i32, i32, i32, i32, vp]
        self.abi = lib.svc_abi_version()
        self.has_out_layout = hasattr(lib, 'svc_render_crops_to_layout')
        if self.has_out_layout:
            lib.svc_render_crops_to_layout.argtypes = [vp, vp, lp, cp, i32, i32, i32, vp, i32, i32, vp, lp, cp, i32, i32, i32, i32, vp]
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


def _up(v, a):
    return (v + a - 1) // a * a


def measure(L, launches, rounds, other=None):
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = {}
    for name, h, w, pitch, coded, (bw, bh) in PICTURES:
        stride = pitch * coded * 3 // 2
        surfaces = torch.randint(0, 256, (N, stride), dtype=torch.uint8, device='cuda')
        lay = _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), NV12, stride, pitch, pitch * coded, pitch)
        rng = np.random.RandomState(0)
        x, y = rng.randint(0, w - bw + 1, N), rng.randint(0, h - bh + 1, N)
        boxes = torch.from_numpy(np.stack([x, y, x + bw, y + bh], 1).astype(np.int32)).cuda()
        for op, (oh, ow), filt in (('9x16_copy', (bh, bw), 0), ('9x16_to_1080x1920_linear', OUT, 0), ('9x16_to_1080x1920_lanczos', OUT, 1)):
            for fmt, fname in ((NV12, 'nv12'), (RGB, 'rgb24')):
                coded_oh = _up(oh, 16)
                if fmt == NV12:
                    opitch = _up(ow, 256)
                    ostride = opitch * coded_oh * 3 // 2
                    olay = _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), NV12, ostride, opitch, opitch * coded_oh, opitch)
                    packed = torch.empty((N, oh * 3 // 2, ow), dtype=torch.uint8, device='cuda')
                else:
                    opitch = _up(3 * ow, 256)
                    ostride = opitch * coded_oh
                    olay = _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), RGB, ostride, opitch, 0, 0)
                    packed = torch.empty((N, oh, ow * 3), dtype=torch.uint8, device='cuda')
                pitched = torch.zeros((N, ostride), dtype=torch.uint8, device='cuda')
                if fmt == NV12:
                    planes = ((torch.as_strided(pitched, (N, oh, ow), (ostride, opitch, 1)), packed[:, :oh]),
                              (torch.as_strided(pitched, (N, oh // 2, ow), (ostride, opitch, 1), opitch * coded_oh), packed[:, oh:]))
                else:
                    planes = ((torch.as_strided(pitched, (N, oh, 3 * ow), (ostride, opitch, 1)), packed),)

                def packed_entry(K=L):
                    K.ok(K.lib.svc_render_crops_colour(K.h, p(surfaces), ctypes.byref(lay), None, N, h, w, p(boxes), bw, bh, p(packed), fmt,
                                                       None, oh, ow, filt, 0, st()))

                def leg_a():
                    L.ok(L.lib.svc_render_crops_to_layout(L.h, p(surfaces), ctypes.byref(lay), None, N, h, w, p(boxes), bw, bh, p(pitched),
                                                          ctypes.byref(olay), None, oh, ow, filt, 0, st()))

                def leg_b():
                    packed_entry()
                    for dst, src in planes:
                        dst.copy_(src)
                legs = dict(c=packed_entry)
                if L.has_out_layout:
                    legs = dict(a=leg_a, b=leg_b, c=packed_entry)
                    leg_a()
                    packed_entry()
                    assert all(torch.equal(dst, src) for dst, src in planes), 'the pitched and the packed output disagree'
                    assert int(pitched.count_nonzero()) <= sum(int(src.numel()) for _, src in planes), 'a byte outside the picture was written'
                if other is not None:
                    legs['c_other'] = lambda: packed_entry(other)
                    packed_entry()
                    want = packed.clone()
                    packed.zero_()
                    legs['c_other']()
                    assert torch.equal(packed, want), 'the two libraries disagree'
                ms = {k: [] for k in legs}
                for r in range(rounds):                             # odd rounds run the legs in reverse order: a leg's place in the
                    order = list(legs.items())                      # sequence (what the leg before it left in the caches) shows in its values
                    for k, fn in (order[::-1] if r & 1 else order):
                        ms[k].append(round(_ms(fn, launches), 4))
                row = dict(out_layout=dict(pitch=opitch, coded_height=coded_oh, frame_stride=ostride), out_bytes_per_32=int(packed.numel()))
                for k, v in ms.items():
                    med = float(np.median(v))
                    row[k] = dict(ms_per_32=v, median=round(med, 4), spread=round((max(v) - min(v)) / med, 4))
                if L.has_out_layout:
                    row['b_over_a'] = round(row['b']['median'] / row['a']['median'], 3)
                    row['a_over_c'] = round(row['a']['median'] / row['c']['median'], 3)
                if other is not None:
                    row['c_over_c_other'] = round(row['c']['median'] / row['c_other']['median'], 4)
                res['%s_%s_to_%s' % (name, op, fname)] = row
                del packed, pitched, planes
        del surfaces
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--with-lib', help='another build, loaded beside this one: its packed entry is leg c_other of the same run')
    ap.add_argument('--out', help='also write the JSON to this file')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = Lib(_lib.LIB_PATH)
    other = Lib(args.with_lib) if args.with_lib else None
    res = dict(method='NV12 surfaces read through their layout, %d-frame batch resident in HBM, 10 warm-up launches, device events over %d '
                      'launches, legs alternated %d times in one process, odd rounds in reverse order; a = svc_render_crops_to_layout into the '
                      'pitched buffer, b = svc_render_crops_colour (packed) + one strided device copy per plane into the same buffer, c = '
                      'svc_render_crops_colour alone, c_other = the other build\'s; out layout: pitch = row bytes rounded up to 256, chroma '
                      'behind the height rounded up to 16; spread = (max - min) / median' % (N, args.launches, args.rounds),
               abi=L.abi, library='this tree', kernels=measure(L, args.launches, args.rounds, other))
    if other is not None:
        res['other_library'] = dict(abi=other.abi, library=os.path.basename(os.path.dirname(os.path.abspath(args.with_lib))), loaded='in this process')
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
