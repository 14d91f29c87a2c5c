#!/usr/bin/env python3
"""The focus stability of the ISM 2021 parameter set (sc_init_crop_params(use_best_settings=True)) by its two routes, SVC_FOCUS =
device (jump statistics from the resident maps: svc_focus_jumps_u8) and host (every filtered map copied to the host and walked
there: the former route, unchanged, hence the baseline).  Two rows, both with best settings:

  stage   the `_focus_stability` stage of smartVidCrop.after_ingest for ONE resident video of --frames selected frames at
          140 x 250 (synthetic frames through the real ingest, tail inside the ingest).  The stage's own clock (sc_register_time):
          a host clock around work that ends in a device-to-host copy, i.e. in a synchronise.
  job     the 200-video job of tools/run_config3.py's shape (RetargetVid frame counts, frames resident in HBM, ratios 1:3 and 3:1,
          dist.crop_job -> crop_videos, --workers lanes): seconds per job.

Routes alternate inside every repeat (other people's work shares the host), after a warm-up of each; medians, and the spread as
min / max and the inter-quartile range.  The results of the two routes are compared on the way: they must be equal.
Needs a GPU; writes one JSON document (default profiles/focus_device.json) and prints it.

  python tools/bench_focus.py [--frames 600] [--stage-repeats 30] [--videos 200] [--job-repeats 5] [--workers 12] [--out FILE]"""
import argparse
import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retargetvid_amd import dist as D, evaluate as E, ops, smartVidCrop as S, synth, weights   # noqa: E402

ROUTES = ('device', 'host')


def summary(xs, unit_scale=1.0, digits=3):
    a = np.sort(np.asarray(xs, np.float64)) * unit_scale
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=round(float(np.median(a)), digits), min=round(float(a[0]), digits), max=round(float(a[-1]), digits),
                iqr=round(float(q3 - q1), digits), n=int(len(a)))


def verdict(rows):
    """The requirement: the device route is not slower than the host route by more than the host route's own spread (its IQR)."""
    d, h = rows['device'], rows['host']
    return dict(device_over_host=round(d['median'] / h['median'], 3), device_minus_host=round(d['median'] - h['median'], 3),
                host_spread_iqr=h['iqr'], device_not_slower_beyond_host_spread=bool(d['median'] - h['median'] <= h['iqr']))


def bench_stage(n_sel, repeats, warmup):
    CP = S.sc_init_crop_params(use_best_settings=True)
    n = n_sel * CP['skip']
    sel = S._select_frames(n, n, [0, n], CP['skip'], CP['read_batch'])[0]
    video = dict(fr=30.0, frame_count=n, w=640, h=360, frames=synth.ResidentBlobVideo(n, sel, seed=1), trans_inds=[0, n])
    eng = ops.Engine(weights.make_synthetic_state_dict(0))
    VD0 = S.ingest_frames(video, CP, engine=eng, stream_batch=64)
    maps = VD0['smaps_dev']
    times, outs = {r: [] for r in ROUTES}, {}
    for k in range(warmup + repeats):
        for route in (ROUTES if k % 2 == 0 else ROUTES[::-1]):
            os.environ['SVC_FOCUS'] = route
            torch.cuda.synchronize()
            S.sc_init_time()
            fresh = {k: (v if k == 'smaps_dev' else copy.deepcopy(v)) for k, v in VD0.items()}      # (the maps are only read: the tail ran)
            VD, _ = S.after_ingest(S._LazySmaps(fresh), CP, eng)
            if k >= warmup:
                times[route].append(S._tls.times['_focus_stability'])
            outs[route] = (VD['jumps'], VD['jumps_inds'], VD['dx'], VD['dy'])
    assert outs['device'] == outs['host'], 'the two routes disagree'
    eng.close()
    rows = {r: summary(times[r], 1e3) for r in ROUTES}
    stats = sum(1 for v in outs['device'][0] if v != 255)
    return dict(what='_focus_stability stage of after_ingest, one resident video', unit='ms', selected_frames=int(maps.shape[0]),
                map_shape=[int(v) for v in maps.shape[1:]], map_bytes=int(maps.numel()), jump_statistics=stats,
                low_saliency_jumps=len(outs['device'][1]), routes=rows, **verdict(rows))


def bench_job(n_videos, repeats, workers):
    annots = E.load_annotations(os.path.join(ROOT, 'tests', 'golden', 'retargetvid'))
    vids = E.VID_INDS[:n_videos]
    counts = [len(annots[0]['1-3'][v]) for v in vids]
    CP = S.sc_init_crop_params(use_best_settings=True)
    resident = {}
    for i in range(len(vids)):
        cuts = synth.retargetvid_cuts(vids[i], counts[i])[:-1]
        sel = S._select_frames(counts[i], counts[i], cuts + [counts[i]], CP['skip'], CP['read_batch'])[0]
        resident[i] = (synth.ResidentBlobVideo(counts[i], sel, seed=vids[i]), cuts, len(sel))
    torch.cuda.synchronize()

    def make(i):
        return lambda: dict(fr=30.0, frame_count=counts[i], w=640, h=360, frames=resident[i][0], trans_inds=resident[i][1] + [counts[i]])

    times, boxes = {r: [] for r in ROUTES}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(1 + repeats):                                     # (repeat 0 of each route pays the one-time costs: not recorded)
            for route in (ROUTES if k % 2 == 0 else ROUTES[::-1]):
                os.environ['SVC_FOCUS'] = route
                allb, st = D.crop_job(make, counts, ['%03d' % v for v in vids], CP, ('1:3', '3:1'), out_dir=os.path.join(tmp, route),
                                      workers=workers, run_name='best')
                if k:
                    times[route].append(st['seconds_rank'])
                boxes[route] = allb
    for ratio in boxes['device']:
        for i in boxes['device'][ratio]:
            assert np.array_equal(boxes['device'][ratio][i], boxes['host'][ratio][i]), 'the two routes disagree (video %d)' % i
    rows = {r: summary(times[r]) for r in ROUTES}
    sel_frames = sum(v[2] for v in resident.values())
    return dict(what='200-video job, best settings, frames resident, dist.crop_job -> crop_videos', unit='s', videos=len(vids),
                workers=workers, video_frames=int(sum(counts)), selected_frames=int(sel_frames),
                map_bytes_host_route_copies=int(sel_frames) * 140 * 250, routes=rows, **verdict(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=600, help='selected frames of the stage row\'s video')
    ap.add_argument('--stage-repeats', type=int, default=30)
    ap.add_argument('--stage-warmup', type=int, default=3)
    ap.add_argument('--videos', type=int, default=200)
    ap.add_argument('--job-repeats', type=int, default=5, help='0 = no job row')
    ap.add_argument('--workers', type=int, default=12)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'focus_device.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_focus.py measures on the GPU: none is visible')
    torch.cuda.set_device(0)
    saved = os.environ.get('SVC_FOCUS')
    try:
        doc = dict(tool='tools/bench_focus.py', device=torch.cuda.get_device_name(0), settings='sc_init_crop_params(use_best_settings=True)',
                   method='routes alternate within every repeat after a warm-up of each; median, min, max and inter-quartile range; '
                          'the two routes\' results are compared and equal',
                   stage=bench_stage(args.frames, args.stage_repeats, args.stage_warmup))
        if args.job_repeats > 0:
            doc['job'] = bench_job(args.videos, args.job_repeats, args.workers)
    finally:
        if saved is None:
            os.environ.pop('SVC_FOCUS', None)
        else:
            os.environ['SVC_FOCUS'] = saved
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fp:
            fp.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
