"""NV12 input against RGB input (svc_resize_frames_nv12 / svc_render_crops_nv12, smartVidCrop._HostFeed): one JSON line.

  * host-fed down-scale to 140x250 (_HostFeed.downscale, 32 frames per call) from a pageable numpy array and from a pinned
    tensor, at 640x360, 1080p and 4K: frames/s and GB/s over PCIe per format -- the median of --regions timed regions
    (each the whole video once, between two synchronisations) after a warm-up region;
  * device-resident: event time per 32-frame launch of the down-scale (three sizes) and of both renderer paths (4K 9:16
    window: copy, and -> 1080x1920) per format, with bytes moved / time beside the 6.3 TB/s achievable HBM bandwidth
    tools/bench_render.py uses.  Bytes moved: the renderer reads its windows (3 bytes per pixel, 1.5 as NV12) and writes
    its output; the down-scale is given as whole source frames per second times their size (it taps 2 x 2 source pixels
    per output pixel, so at 4K it touches a fraction of the frame: the figure is what a streaming reader would need).

The rgb24 legs use nothing the tree had before NV12 input existed, so `--formats rgb24` runs unchanged on the commit before
it: that run is the baseline, and `--baseline FILE` (its JSON line) is embedded under "parent" with the ratios that matter.

usage: python tools/bench_nv12.py [--formats rgb24,nv12] [--regions 5] [--launches 50] [--baseline parent.json] [--out FILE]
A rocprofv3 --kernel-trace --stats run of its own gives the per-kernel durations without the event overhead."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from retargetvid_amd import ops, smartVidCrop as S  # noqa: E402

HBM_TBS = 6.3
SAL_H, SAL_W = 140, 250
SIZES = (('640x360', 360, 640, 512), ('1920x1080', 1080, 1920, 128), ('3840x2160', 2160, 3840, 64))   # name, h, w, frames of the host video


def frame_shape(fmt, h, w):
    return (h * 3 // 2, w) if fmt == 'nv12' else (h, w, 3)


def host_video(fmt, h, w, n):
    """n frames of noise (16 distinct ones, repeated: the bytes do not matter to the copy, generating them does to the run time)."""
    base = np.random.RandomState(h).randint(0, 256, (16,) + frame_shape(fmt, h, w), dtype=np.uint8)
    return np.concatenate([base] * (n // 16))


def host_fed(eng, fmt, regions):
    out = {}
    for name, h, w, n in SIZES:
        frames = host_video(fmt, h, w, n)
        nbytes = int(np.prod(frames.shape[1:]))
        for src_name in ('pageable', 'pinned'):
            src = frames if src_name == 'pageable' else torch.from_numpy(frames).pin_memory()
            feed = S._HostFeed(eng)

            def region():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(0, n, 32):
                    idx = list(range(s, min(n, s + 32)))
                    if fmt == 'nv12':
                        feed.downscale(src, idx, SAL_H, SAL_W, pix_fmt='nv12')
                    else:
                        feed.downscale(src, idx, SAL_H, SAL_W)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            region()                                                   # warm-up: staging buffers, code objects, the table
            ts = sorted(region() for _ in range(regions))
            med = ts[len(ts) // 2]
            out['%s_%s' % (name, src_name)] = dict(frames=n, bytes_per_frame=nbytes, stage_frames=feed.k, fps=round(n / med, 1),
                                                   pcie_gbs=round(n * nbytes / med / 1e9, 2), region_s=[round(t, 5) for t in ts])
            del feed, src
            torch.cuda.empty_cache()
        del frames
    return out


def _timed(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def device_resident(eng, fmt, launches):
    out = {}
    n = 32
    for name, h, w, _ in SIZES:
        frames = torch.randint(0, 256, (n,) + frame_shape(fmt, h, w), dtype=torch.uint8, device=eng.device)
        fn = (lambda: eng.resize_frames(frames, SAL_H, SAL_W, pix_fmt='nv12')) if fmt == 'nv12' else (lambda: eng.resize_frames(frames, SAL_H, SAL_W))
        ms = _timed(fn, launches)
        src = frames.numel()
        out['downscale_%s' % name] = dict(ms_per_32=round(ms, 4), fps=round(n / ms * 1e3), source_bytes_per_frame=src // n,
                                          source_tbs=round(src / (ms * 1e-3) / 1e12, 3), frac_of_hbm=round(src / (ms * 1e-3) / 1e12 / HBM_TBS, 3))
        if name == '3840x2160':
            bw, bh = 1215, 2160
            rng = np.random.RandomState(0)
            x, y = rng.randint(0, w - bw + 1, n), rng.randint(0, h - bh + 1, n)
            boxes = torch.from_numpy(np.stack([x, y, x + bw, y + bh], 1).astype(np.int32)).to(eng.device)
            for tag, (ow, oh) in (('copy', (bw, bh)), ('to_1080x1920', (1080, 1920))):
                dst = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=eng.device)
                fn = (lambda: eng._render(frames, boxes, bw, bh, dst, False, 'nv12')) if fmt == 'nv12' else (lambda: eng._render(frames, boxes, bw, bh, dst, False))
                ms = _timed(fn, launches)
                moved = n * (bw * bh * 3 // (2 if fmt == 'nv12' else 1) + ow * oh * 3)
                out['render_4k_9x16_%s' % tag] = dict(ms_per_32=round(ms, 4), us_per_frame=round(ms * 1e3 / n, 2), bytes_per_frame=moved // n,
                                                      eff_tbs=round(moved / (ms * 1e-3) / 1e12, 3),
                                                      frac_of_hbm=round(moved / (ms * 1e-3) / 1e12 / HBM_TBS, 3))
                del dst
        del frames
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--formats', default='rgb24,nv12')
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--skip-device', action='store_true')
    ap.add_argument('--baseline', default=None, help='JSON line of a `--formats rgb24` run on the commit before NV12 input')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.regions < 5:
        ap.error('--regions: at least 5 timed regions')
    torch.cuda.set_device(0)
    eng = ops.Engine(device=0)
    res = dict(sal_size=[SAL_H, SAL_W], regions=args.regions, launches=args.launches, hbm_tbs=HBM_TBS)
    for fmt in args.formats.split(','):
        res[fmt] = {}
        if not args.skip_host:
            res[fmt]['host_fed'] = host_fed(eng, fmt, args.regions)
        if not args.skip_device:
            res[fmt]['device'] = device_resident(eng, fmt, args.launches)
    eng.close()
    if args.baseline:
        with open(args.baseline) as fp:
            parent = json.loads(fp.read().strip().splitlines()[-1])
        res['parent'] = parent
        if not args.skip_host and 'host_fed' in parent.get('rgb24', {}):
            ratio = {}
            for k, v in parent['rgb24']['host_fed'].items():
                ratio[k] = dict(rgb24_new_over_parent=round(res['rgb24']['host_fed'][k]['fps'] / v['fps'], 3) if 'rgb24' in res else None,
                                nv12_over_parent_rgb24=round(res['nv12']['host_fed'][k]['fps'] / v['fps'], 3) if 'nv12' in res else None)
            res['host_fed_fps_ratio'] = ratio
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(line + '\n')


if __name__ == '__main__':
    main()
