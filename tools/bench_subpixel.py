"""Sub-pixel windows (svc_render_windows_q8) against the integer entry on the same windows: one JSON line, and
profiles/render_subpixel.json with --out.

A 32-frame batch resident in HBM, the pictures of profiles/pitched_output.json: 1920 x 1080 and 3840 x 2160, as packed RGB frames and
as NV12 decoder surfaces (pitch 2048 / coded height 1088; 4096 / 2176) read where they lie; the 9:16 window (607 x 1080; 1215 x
2160) resampled to 1080 x 1920, to packed RGB and to packed NV12.  Legs, over the same buffers:
  q8         svc_render_windows_q8 at origins with random phases (x and y where the window can move)
  q8_whole   the same entry at the whole-pixel origins of leg int (phase 0: no extra column is tapped)
  int        svc_render_crops_to_layout (SVC_FILTER_LINEAR) with the boxes (xi, yi, xi + bw, yi + bh) of those origins
  int_other  the integer entry of ANOTHER build (--with-lib, e.g. the parent commit's library) loaded into the same process with a
             handle of its own
10 warm-up launches, device events over --launches launches, the legs alternated --rounds times in one process (odd rounds in
reverse order); per leg the values, their median and spread = (max - min) / median.  Before timing, leg q8_whole's bytes are
compared with leg int's, and leg int_other's with leg int's.

usage: python tools/bench_subpixel.py [--launches 100] [--rounds 9] [--with-lib other.so] [--out file.json]"""
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
PICTURES = (('1920x1080', 1080, 1920, 2048, 1088, (607, 1080)),
            ('3840x2160', 2160, 3840, 4096, 2176, (1215, 2160)))
OUT = (1920, 1080)               # (rows, columns)
NV12, RGB = 1, 0


class Lib:
    """The render entries of a libsvc_hip.so that has svc_render_crops_to_layout (and, this tree's, svc_render_windows_q8)."""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        lp, cp = ctypes.POINTER(_lib.SvcFrameLayout), ctypes.POINTER(_lib.SvcColour)
        lib.svc_last_error.restype = ctypes.c_char_p
        lib.svc_create.argtypes = [vp, ctypes.c_size_t, i32, ctypes.POINTER(vp)]
        lib.svc_destroy.argtypes = [vp]
        lib.svc_render_crops_to_layout.argtypes = [vp, vp, lp, cp, i32, i32, i32, vp, i32, i32, vp, lp, cp, i32, i32, i32, i32, vp]
        self.abi = lib.svc_abi_version()
        self.has_q8 = hasattr(lib, 'svc_render_windows_q8')
        if self.has_q8:
            lib.svc_render_windows_q8.argtypes = [vp, vp, lp, cp, i32, i32, i32, vp, i32, i32, vp, lp, cp, i32, i32, i32, vp]
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


def _layout(fmt, stride, pitch, coff, cpitch):
    return _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), fmt, stride, pitch, coff, cpitch)


def measure(L, launches, rounds, other=None):
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    oh, ow = OUT
    res = {}
    for name, h, w, pitch, coded, (bw, bh) in PICTURES:
        rng = np.random.RandomState(0)
        q8 = np.stack([rng.randint(0, (w - bw) * 256 + 1, N), rng.randint(0, (h - bh) * 256 + 1, N)], 1)
        whole = q8 >> 8
        org = torch.from_numpy(q8.astype(np.int32)).cuda()
        org_whole = torch.from_numpy((whole << 8).astype(np.int32)).cuda()
        boxes = torch.from_numpy(np.concatenate([whole, whole + [bw, bh]], 1).astype(np.int32)).cuda()
        for in_fmt, in_name in ((RGB, 'rgb24'), (NV12, 'nv12')):
            if in_fmt == NV12:
                stride = pitch * coded * 3 // 2
                lay = _layout(NV12, stride, pitch, pitch * coded, pitch)
            else:
                stride = 3 * w * h
                lay = _layout(RGB, stride, 3 * w, 0, 0)
            frames = torch.randint(0, 256, (N, stride), dtype=torch.uint8, device='cuda')
            for out_fmt, out_name in ((RGB, 'rgb24'), (NV12, 'nv12')):
                if out_fmt == NV12:
                    olay = _layout(NV12, ow * oh * 3 // 2, ow, ow * oh, ow)
                    out = torch.empty((N, oh * 3 // 2, ow), dtype=torch.uint8, device='cuda')
                else:
                    olay = _layout(RGB, 3 * ow * oh, 3 * ow, 0, 0)
                    out = torch.empty((N, oh, ow * 3), dtype=torch.uint8, device='cuda')

                def integer(K=L):
                    K.ok(K.lib.svc_render_crops_to_layout(K.h, p(frames), ctypes.byref(lay), None, N, h, w, p(boxes), bw, bh, p(out),
                                                          ctypes.byref(olay), None, oh, ow, 0, 0, st()))

                def windows(o=org):
                    L.ok(L.lib.svc_render_windows_q8(L.h, p(frames), ctypes.byref(lay), None, N, h, w, p(o), bw, bh, p(out), ctypes.byref(olay),
                                                     None, oh, ow, 0, st()))
                integer()
                want = out.clone()
                legs = dict(int=integer)
                if L.has_q8:
                    legs = dict(q8=windows, q8_whole=lambda: windows(org_whole), int=integer)
                    out.zero_()
                    legs['q8_whole']()
                    assert torch.equal(out, want), 'whole-pixel origins and the integer entry disagree'
                    windows()
                    assert not torch.equal(out, want), 'the phases change nothing'
                if other is not None:
                    legs['int_other'] = lambda: integer(other)
                    out.zero_()
                    legs['int_other']()
                    assert torch.equal(out, want), 'the two libraries disagree'
                ms = {k: [] for k in legs}
                for r in range(rounds):                             # odd rounds run the legs in reverse order
                    order = list(legs.items())
                    for k, fn in (order[::-1] if r & 1 else order):
                        ms[k].append(round(_ms(fn, launches), 4))
                row = dict(out_bytes_per_32=int(out.numel()))
                for k, v in ms.items():
                    med = float(np.median(v))
                    row[k] = dict(ms_per_32=v, median=round(med, 4), spread=round((max(v) - min(v)) / med, 4))
                if L.has_q8:
                    row['q8_over_int'] = round(row['q8']['median'] / row['int']['median'], 4)
                    row['q8_whole_over_int'] = round(row['q8_whole']['median'] / row['int']['median'], 4)
                if other is not None:
                    row['int_over_int_other'] = round(row['int']['median'] / row['int_other']['median'], 4)
                res['%s_%s_9x16_to_1080x1920_%s' % (name, in_name, out_name)] = row
                del out, want
            del frames
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--with-lib', help='another build, loaded beside this one: its integer entry is leg int_other of the same run')
    ap.add_argument('--out', help='also write the JSON to this file')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = Lib(_lib.LIB_PATH)
    other = Lib(args.with_lib) if args.with_lib else None
    res = dict(method='%d-frame batch resident in HBM (packed RGB frames; NV12 surfaces read through their layout), 10 warm-up launches, device '
                      'events over %d launches, legs alternated %d times in one process, odd rounds in reverse order; q8 = svc_render_windows_q8 '
                      'at origins with random phases, q8_whole = the same at whole-pixel origins, int = svc_render_crops_to_layout (linear) '
                      'with the boxes of those origins, int_other = the other build\'s; packed outputs; spread = (max - min) / median'
                      % (N, args.launches, args.rounds),
               abi=L.abi, library='this tree', kernels=measure(L, args.launches, args.rounds, other))
    if other is not None:
        res['other_library'] = dict(abi=other.abi, library=os.path.basename(args.with_lib), loaded='in this process')
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
