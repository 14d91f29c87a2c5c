"""Rendering on the device (svc_render_crops_u8, render.render_video): one JSON line.

  * per geometry: kernel time of a 32-frame batch resident in HBM (device events over --launches launches after a
    warm-up), and the effective bandwidth = (bytes of the source windows read + bytes written) / kernel time, against the
    6.3 TB/s achievable HBM bandwidth of the MI355X;
  * render_video from host memory: frames/s for a --frames-frame 1080p numpy video (native 9:16 windows), beside the bare
    H2D of the frames and D2H of the crops (same bytes, same pinned-buffer sizes) timed in the same run.

  * --nv12-out: the NV12-output entries (svc_render_crops_u8_to_nv12 / _nv12_to_nv12) beside the RGB-output ones, same
    geometries, both sources, same method; and render_video end to end on the host-fed 1080p case with RGB and with NV12
    output.  The two outputs alternate --rounds times in one process, so that the run-to-run spread is visible next to
    their difference.

  * --lanczos: the Lanczos filter (svc_render_crops_filter) on the two deliverable shapes, RGB and NV12 output each, beside
    three references measured in the same process: (a) the linear path on the same shape, (b) a device-to-device copy of
    the output's bytes (the write floor), (c) what a user does without it: native-size device crop, D2H, PIL resize(LANCZOS)
    on 16 host threads.  Also the band B the launcher picks and its horizontal-pass redundancy sum(tile rows) / bh.

usage: python tools/bench_render.py [--launches 200] [--frames 300] [--nv12-out [--rounds 3]] [--lanczos] [--out file.json]
A rocprofv3 --kernel-trace --stats run of its own gives the per-kernel durations without the event overhead."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from retargetvid_amd import ops, render  # noqa: E402

HBM_TBS = 6.3

GEOMETRIES = (  # name, (h, w) frame, (bw, bh) window, (ow, oh) output or None
    ('640x360_1x3_copy', (360, 640), (120, 360), None),
    ('1920x1080_9x16_copy', (1080, 1920), (608, 1080), None),
    ('1920x1080_9x16_to_1080x1920', (1080, 1920), (608, 1080), (1080, 1920)),
    ('3840x2160_9x16_to_1080x1920', (2160, 3840), (1215, 2160), (1080, 1920)),
)


def boxes_for(n, h, w, bw, bh, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, w - bw + 1, n)
    y = rng.randint(0, h - bh + 1, n)
    return np.stack([x, y, x + bw, y + bh], 1).astype(np.int32)


def kernel_times(eng, launches):
    out = {}
    n = 32
    for name, (h, w), (bw, bh), osz in GEOMETRIES:
        frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=eng.device)
        boxes = torch.from_numpy(boxes_for(n, h, w, bw, bh)).to(eng.device)
        ow, oh = osz or (bw, bh)
        dst = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=eng.device)
        for _ in range(10):
            eng._render(frames, boxes, bw, bh, dst, False)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            eng._render(frames, boxes, bw, bh, dst, False)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / launches
        moved = n * (bw * bh * 3 + ow * oh * 3)
        out[name] = dict(ms_per_32=round(ms, 4), us_per_frame=round(ms * 1e3 / n, 2), bytes_per_frame=moved // n,
                         eff_tbs=round(moved / (ms * 1e-3) / 1e12, 3), frac_of_hbm=round(moved / (ms * 1e-3) / 1e12 / HBM_TBS, 3))
        del frames, dst
        torch.cuda.empty_cache()
    return out


def _event_ms(fn, launches):
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


def nv12_out_kernel_times(eng, launches, rounds):
    """Per geometry and source: ms per 32-frame launch with RGB output and with NV12 output, `rounds` values each, measured
    alternately; bytes per frame = window bytes read (in the source's format) + bytes written."""
    out = {}
    n = 32
    for name, (h, w), (bw, bh), osz in GEOMETRIES:
        ow, oh = osz or (bw, bh)
        boxes = torch.from_numpy(boxes_for(n, h, w, bw, bh)).to(eng.device)
        for src in ops.PIX_FMTS:
            frames = torch.randint(0, 256, (n,) + ops.frame_shape(src, h, w), dtype=torch.uint8, device=eng.device)
            dst = {f: torch.empty((n,) + ops.frame_shape(f, oh, ow), dtype=torch.uint8, device=eng.device) for f in ops.OUT_FMTS}
            ms = {f: [] for f in ops.OUT_FMTS}
            for _ in range(rounds):
                for f in ops.OUT_FMTS:
                    ms[f].append(round(_event_ms(lambda: eng._render(frames, boxes, bw, bh, dst[f], False, src, f), launches), 4))
            px_in = 3.0 if src == 'rgb24' else 1.5
            row = dict(ms_per_32_rgb_out=ms['rgb24'], ms_per_32_nv12_out=ms['nv12'],
                       nv12_over_rgb=round(float(np.median(ms['nv12']) / np.median(ms['rgb24'])), 3))
            for f, px_out in (('rgb24', 3.0), ('nv12', 1.5)):
                moved = n * (bw * bh * px_in + ow * oh * px_out)
                row['bytes_per_frame_%s_out' % f.replace('24', '')] = int(moved // n)
                row['eff_tbs_%s_out' % f.replace('24', '')] = round(moved / (float(np.median(ms[f])) * 1e-3) / 1e12, 3)
            out['%s_from_%s' % (name, src)] = row
            del frames, dst
            torch.cuda.empty_cache()
    return out


def nv12_out_host_fed(eng, nf, rounds):
    """render_video end to end, host-fed 1080p numpy at native 608 x 1080 windows: seconds with RGB and with NV12 output,
    alternating."""
    h, w, bw, bh = 1080, 1920, 608, 1080
    frames = np.random.RandomState(1).randint(0, 256, (nf, h, w, 3), dtype=np.uint8)
    VD = dict(fc=nf, bbs_np=boxes_for(nf, h, w, bw, bh, seed=2).astype(np.int64))
    sink = lambda c: None
    secs = {f: [] for f in ops.OUT_FMTS}
    for f in ops.OUT_FMTS:                                        # warm-up (buffers of both formats' sizes)
        render.render_video(frames[:40], dict(fc=40, bbs_np=VD['bbs_np'][:40]), engine=eng, sink=sink, out_fmt=f)
    for _ in range(rounds):
        for f in ops.OUT_FMTS:
            render.render_video(frames[:40], dict(fc=40, bbs_np=VD['bbs_np'][:40]), engine=eng, sink=sink, out_fmt=f)   # (the ring is re-made per format)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            render.render_video(frames, VD, engine=eng, sink=sink, out_fmt=f)
            torch.cuda.synchronize()
            secs[f].append(round(time.perf_counter() - t0, 4))
    return dict(frames=nf, render_s_rgb_out=secs['rgb24'], render_s_nv12_out=secs['nv12'],
                fps_rgb_out=round(nf / float(np.median(secs['rgb24'])), 1), fps_nv12_out=round(nf / float(np.median(secs['nv12'])), 1),
                d2h_bytes_per_frame=dict(rgb_out=bw * bh * 3, nv12_out=bw * bh * 3 // 2))


LANCZOS_SHAPES = (  # name, source format, (h, w) frame, (bw, bh) window, (ow, oh) output
    ('1080p_607x1080_to_1080x1920', 'rgb24', (1080, 1920), (607, 1080), (1080, 1920)),
    ('4k_nv12_1215x2160_to_720x1280', 'nv12', (2160, 3840), (1215, 2160), (720, 1280)),
)


def lanczos_band(bw, bh, oh, ow, out_fmt):
    """The launcher's rule (include/svc.h) restated: -> (B, tile rows T(B), LDS bytes, sum(tile rows) / bh)."""
    from oracle import lanczos_ref
    up16 = lambda v: (v + 15) // 16 * 16
    R = 2 if out_fmt == 'nv12' else 1
    D = 2 * up16(3 * ow) + 3 * (up16(ow) + 16) if out_fmt == 'nv12' else 3 * ow + 16
    vb = lanczos_ref.precompute_coeffs(bh, oh)[0].astype(int) if bh != oh else np.stack([np.arange(oh), np.ones(oh, int)], 1)
    rows = lambda B: [int((vb[y:y + B, 0] + vb[y:y + B, 1]).max() - vb[y:y + B, 0].min()) for y in range(0, oh, B)]
    B = min(32, (oh + R - 1) // R * R) // R * R
    while 2 * up16(3 * bw + 32) + max(rows(B)) * up16(3 * ow) + D > 65536:
        B -= R
    t = rows(B)
    return B, max(t), 2 * up16(3 * bw + 32) + max(t) * up16(3 * ow) + D, round(sum(t) / bh, 3)


def lanczos_times(eng, launches, rounds):
    """Per shape and output format: ms per 32-frame launch of the Lanczos filter, of the linear filter and of a D2D copy of
    the output bytes, `rounds` values each, measured alternately; per shape, once: the host route (device crop at native
    size, D2H into pinned memory, PIL resize(LANCZOS) of the 32 crops on 16 threads), ms per 32 frames."""
    from concurrent.futures import ThreadPoolExecutor
    out = {}
    n = 32
    for name, src, (h, w), (bw, bh), (ow, oh) in LANCZOS_SHAPES:
        frames = torch.randint(0, 256, (n,) + ops.frame_shape(src, h, w), dtype=torch.uint8, device=eng.device)
        boxes = torch.from_numpy(boxes_for(n, h, w, bw, bh)).to(eng.device)
        px_in = 3.0 if src == 'rgb24' else 1.5
        for f, px_out in (('rgb24', 3.0), ('nv12', 1.5)):
            dst = torch.empty((n,) + ops.frame_shape(f, oh, ow), dtype=torch.uint8, device=eng.device)
            twin = torch.empty_like(dst)
            runs = dict(lanczos=lambda: eng._render(frames, boxes, bw, bh, dst, False, src, f, None, 'lanczos'),
                        linear=lambda: eng._render(frames, boxes, bw, bh, dst, False, src, f),
                        d2d_copy=lambda: twin.copy_(dst))
            ms = {k: [] for k in runs}
            for _ in range(rounds):
                for k, fn in runs.items():
                    ms[k].append(round(_event_ms(fn, launches), 4))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            B, T, lds, red = lanczos_band(bw, bh, oh, ow, f)
            moved = n * (bw * bh * px_in + ow * oh * px_out)
            out['%s_%s_out' % (name, f.replace('24', ''))] = dict(
                ms_per_32_lanczos=ms['lanczos'], ms_per_32_linear=ms['linear'], ms_per_32_d2d_copy_of_output=ms['d2d_copy'],
                lanczos_over_linear=round(med['lanczos'] / med['linear'], 3), lanczos_over_d2d_copy=round(med['lanczos'] / med['d2d_copy'], 3),
                us_per_frame_lanczos=round(med['lanczos'] * 1e3 / n, 2), bytes_per_frame=int(moved // n),
                eff_tbs_lanczos=round(moved / (med['lanczos'] * 1e-3) / 1e12, 3),
                band_rows=B, tile_rows=T, lds_bytes=lds, horizontal_pass_redundancy=red)
            del dst, twin
        try:
            from PIL import Image
        except ImportError:
            out[name + '_host_route'] = None
        else:
            crops = torch.empty((n, bh, bw, 3), dtype=torch.uint8, device=eng.device)
            pinned = torch.empty((n, bh, bw, 3), dtype=torch.uint8).pin_memory()
            pool = ThreadPoolExecutor(16)
            secs = []
            for _ in range(rounds + 1):                              # (the first round is the warm-up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng._render(frames, boxes, bw, bh, crops, False, src, 'rgb24')
                pinned.copy_(crops, non_blocking=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                host = pinned.numpy()
                list(pool.map(lambda c: np.asarray(Image.fromarray(c).resize((ow, oh), Image.LANCZOS)), host))
                secs.append((round((t1 - t0) * 1e3, 3), round((time.perf_counter() - t1) * 1e3, 3)))
            pool.shutdown()
            out[name + '_host_route'] = dict(ms_per_32_crop_and_d2h=[a for a, _ in secs[1:]], ms_per_32_pillow_16_threads=[b for _, b in secs[1:]],
                                             ms_per_32=round(float(np.median([a + b for a, b in secs[1:]])), 3), output='rgb24')
            del crops, pinned
        del frames
        torch.cuda.empty_cache()
    return out


def host_fed(eng, nf):
    h, w, bw, bh = 1080, 1920, 608, 1080
    frames = np.random.RandomState(1).randint(0, 256, (nf, h, w, 3), dtype=np.uint8)
    VD = dict(fc=nf, bbs_np=boxes_for(nf, h, w, bw, bh, seed=2).astype(np.int64))
    sink = lambda c: None
    render.render_video(frames[:40], dict(fc=40, bbs_np=VD['bbs_np'][:40]), engine=eng, sink=sink)       # warm-up (buffers)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    render.render_video(frames, VD, engine=eng, sink=sink)
    torch.cuda.synchronize()
    t_render = time.perf_counter() - t0
    # the bare copies of the same bytes through pinned buffers of the same sizes (15 frames in, 32 crops out), serial
    k_in, k_out = 15, 32
    pin_in = torch.empty((k_in, h, w, 3), dtype=torch.uint8).pin_memory()
    dev_in = torch.empty((k_in, h, w, 3), dtype=torch.uint8, device=eng.device)
    pin_out = torch.empty((k_out, bh, bw, 3), dtype=torch.uint8).pin_memory()
    dev_out = torch.empty((k_out, bh, bw, 3), dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, nf, k_in):
        m = min(k_in, nf - s)
        pin_in[:m].numpy()[...] = frames[s:s + m]
        dev_in[:m].copy_(pin_in[:m], non_blocking=True)
        torch.cuda.synchronize()
    t_h2d = time.perf_counter() - t0
    t0 = time.perf_counter()
    for s in range(0, nf, k_out):
        m = min(k_out, nf - s)
        pin_out[:m].copy_(dev_out[:m], non_blocking=True)
        torch.cuda.synchronize()
    t_d2h = time.perf_counter() - t0
    return dict(frames=nf, render_s=round(t_render, 4), fps=round(nf / t_render, 1), bare_h2d_s=round(t_h2d, 4),
                bare_d2h_s=round(t_d2h, 4), render_over_bare=round(t_render / (t_h2d + t_d2h), 3),
                render_over_h2d=round(t_render / t_h2d, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--nv12-out', action='store_true', help='measure the NV12-output entries beside the RGB-output ones')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lanczos', action='store_true', help='measure the Lanczos filter beside the linear one, a D2D copy and the host route')
    ap.add_argument('--out', help='also write the JSON to this file')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    eng = ops.Engine(device=0)
    if args.lanczos:
        res = dict(method='32-frame batch resident in HBM, 10 warm-up launches, device events over %d launches; the Lanczos filter, the '
                          'linear filter and a device-to-device copy of the output alternated %d times in one process; host route: wall '
                          'clock, %d rounds after one warm-up' % (args.launches, args.rounds, args.rounds),
                   lanczos=lanczos_times(eng, args.launches, args.rounds))
    elif args.nv12_out:
        res = dict(method='32-frame batch resident in HBM, 10 warm-up launches, device events over %d launches; RGB and NV12 output '
                          'alternated %d times in one process' % (args.launches, args.rounds),
                   kernels=nv12_out_kernel_times(eng, args.launches, args.rounds))
        if not args.skip_host:
            res['host_fed_1080p_9x16'] = nv12_out_host_fed(eng, args.frames, args.rounds)
    else:
        res = dict(kernels=kernel_times(eng, args.launches))
        if not args.skip_host:
            res['host_fed_1080p_9x16'] = host_fed(eng, args.frames)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as fp:
            json.dump(res, fp, indent=1)
            fp.write('\n')
    eng.close()


if __name__ == '__main__':
    main()
