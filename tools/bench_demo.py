"""The demo video (render.render_demo) against the plain render of the same frames at the same size (render.render_video): one
JSON line, and profiles/demo_video.json with --out.

One 1920 x 1080 video of --frames frames (>= 600), 32 distinct random pictures repeated, once as a numpy array in host memory
(host-fed: gathered into pinned double buffers, H2D on a side stream) and once as a CUDA tensor (device-resident).  Legs, over the
same container, engine and VD:
  video   render_video(video, VD, out_size=(w_process, h_process)) with every window the whole frame: the frames are fed the same
          way and the first device pass is the same full-frame INTER_LINEAR resize to 250 x 140; 105 000 bytes per frame come back
  demo    render_demo(video, VD, CP): that resize, then one svc_demo_frames_u8 launch per chunk; 525 000 bytes per frame come back
Both with a sink that drops the chunks, chunk = 32, the call timed on the host from entry to return (its last D2H has landed).  The
VD is synthetic and deterministic -- fr 25, one map per 6 frames, random raw and filtered maps resident on the device, a random walk
of centres, a jump score below the threshold every 40 maps, a cut every 150 frames -- so the run needs no network pass; its mark
lists are those of render.demo_marks (41 marks on a typical frame).  One warm-up call per leg, then the legs alternated --rounds
times in one process (odd rounds in reverse order); per leg the values, their median and spread = (max - min) / median.
compositor: ops.demo_frames alone on 32 resident small frames, device events over --launches launches, 10 warm-up launches.

usage: python tools/bench_demo.py [--frames 600] [--rounds 9] [--launches 200] [--out profiles/demo_video.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retargetvid_amd import ops, render, smartVidCrop as S  # noqa: E402

H, W, PH, PW = 1080, 1920, 140, 250


def synthetic_vd(fc, dev):
    rng = np.random.RandomState(0)
    m = [i // 6 for i in range(fc)]
    n_maps = m[-1] + 1
    walk = lambda lo, hi: np.clip(np.cumsum(rng.randint(-6, 7, n_maps)) + (lo + hi) // 2, lo, hi).astype(np.float64) + 0.5
    dx, dy = walk(5, PW - 6), walk(5, PH - 6)
    dxnf = dx.copy()
    dxnf[::9] += 7.0
    jumps = np.full(n_maps, 255.0)
    jumps[::40] = 12.0
    jumps[1::7] = rng.randint(60, 255, len(jumps[1::7]))
    boxes = np.tile(np.array([[0, 0, W, H]], np.int64), (fc, 1))
    raw = torch.randint(0, 256, (n_maps, PH, PW), dtype=torch.uint8, device=dev)
    return dict(fr=25.0, fc=fc, inds_to_orig=m, h_process=PH, w_process=PW, h_orig=H, w_orig=W, dx=dx.tolist(), dy=dy.tolist(),
                dxnf=dxnf.tolist(), dynf=dy.tolist(), jumps=jumps.tolist(), segm_backup=np.array([[s, min(fc, s + 150) - 1] for s in range(0, fc, 150)]),
                dxs=(np.repeat(dx, 6)[:fc] * W / PW).tolist(), dys=(np.repeat(dy, 6)[:fc] * H / PH).tolist(), bbs_np=boxes, bbs=boxes.tolist(),
                smaps_orig_dev=raw, smaps_dev=torch.where(raw < 150, torch.zeros_like(raw), raw))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=600)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', help='also write the JSON to this file')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = ops.Engine()
    CP = S.sc_init_crop_params(use_best_settings=True)
    fc = args.frames
    VD = synthetic_vd(fc, eng.device)
    marks, first, _ = render.demo_marks(VD, CP)
    base = np.random.RandomState(1).randint(0, 256, (32, H, W, 3)).astype(np.uint8)
    host = np.concatenate([base] * ((fc + 31) // 32))[:fc]
    drop = lambda chunk: None
    res = dict(method=__doc__.split('\n\n')[1].replace('\n', ' '), frames=fc, picture='%dx%d' % (W, H), process='%dx%d' % (PW, PH),
               marks_per_frame=dict(mean=round(float(np.diff(first).mean()), 2), max=int(np.diff(first).max())),
               bytes_per_frame=dict(h2d=H * W * 3, d2h_video=PH * PW * 3, d2h_demo=PH * PW * 15))
    for feed, cont in (('host_fed', host), ('device_resident', None)):
        if cont is None:
            cont = torch.from_numpy(host).to(eng.device)
        legs = dict(video=lambda: render.render_video(cont, VD, engine=eng, out_size=(PW, PH), sink=drop, chunk=32),
                    demo=lambda: render.render_demo(cont, VD, CP, engine=eng, sink=drop, chunk=32))
        for fn in legs.values():
            fn()
        ms = {k: [] for k in legs}
        for r in range(args.rounds):
            order = list(legs.items())
            for k, fn in (order[::-1] if r & 1 else order):
                ms[k].append(round(timed(fn), 3))
        row = {}
        for k, v in ms.items():
            med = float(np.median(v))
            row[k] = dict(ms=v, median=round(med, 3), ms_per_frame=round(med / fc, 4), spread=round((max(v) - min(v)) / med, 4))
        row['demo_over_video'] = round(row['demo']['median'] / row['video']['median'], 4)
        res[feed] = row
        del cont, legs
        torch.cuda.empty_cache()
    res['host_fed']['allowance'] = 1.25
    res['host_fed']['within_allowance'] = bool(res['host_fed']['demo_over_video'] <= 1.25)
    # the compositor alone
    small = torch.randint(0, 256, (32, PH, PW, 3), dtype=torch.uint8, device=eng.device)
    atlas, _ = render.demo_atlas()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in (np.asarray(VD['inds_to_orig'][:32], np.int32), marks, first[:33], atlas)]
    out = torch.empty((32, PH, 5 * PW, 3), dtype=torch.uint8, device=eng.device)
    call = lambda: ops.demo_frames(small, VD['smaps_orig_dev'], VD['smaps_dev'], dev[0], dev[1], dev[2], dev[3], out=out)
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    vals = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            call()
        b.record()
        torch.cuda.synchronize()
        vals.append(round(a.elapsed_time(b) / args.launches * 1e3, 2))
    med = float(np.median(vals))
    res['compositor'] = dict(us_per_32_frames=vals, median=round(med, 2), spread=round((max(vals) - min(vals)) / med, 4),
                             bytes_per_32=dict(read=32 * PH * PW * 5, written=32 * PH * PW * 15),
                             note='events around %d back-to-back launches through ops.demo_frames: includes the host cost of a launch where '
                                  'the kernel is shorter than it' % args.launches)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fp:
            json.dump(res, fp, indent=1)
            fp.write('\n')
    eng.close()


if __name__ == '__main__':
    main()
