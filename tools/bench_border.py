"""Border detection on the device (svc_border_profile_u8, svc_saliency_profile_u8): one JSON line.

  (a) the standalone kernel on 32, 300 and 1 800 raw maps of 140 x 250: device-event time per launch over --launches launches
      after a warm-up, and bytes read / time beside the 6.3 TB/s achievable HBM bandwidth of the MI355X (tools/bench_render.py's
      figure).  At 32 maps (1.1 MB) the launch is what is measured, not the memory system;
  (b) the network's last class ('smooth': k_smooth_down + the quantising kernel) per 32-frame pass of 140 x 250 maps with and
      without the profile (svc_profile_enable on the class), alternating;
  (c) the 200-video job (tools/run_config3.py in child processes, --repeat runs each after one that pays the one-time costs)
      with t_border = -1 and with --t-border.

usage: python tools/bench_border.py [--launches 300] [--videos 200] [--repeat 3] [--t-border 90] [--out profiles/border_detection.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def job(videos, repeat, t_border, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'run_config3.py'), '--videos', str(videos), '--repeat', str(repeat + 1),
           '--t-border', str(t_border), '--out', out_dir]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    if p.returncode != 0 or not lines:
        raise RuntimeError('run_config3 failed (%d):\n%s' % (p.returncode, p.stdout[-2000:]))
    d = json.loads(lines[-1])
    return dict(t_border=t_border, seconds_runs=d['seconds_rank0_runs'][1:], first_run_s=d['seconds_rank0_runs'][0],
                chunks=d['scheduler'].get('chunks'), saliency_frames=d['saliency_frames_rank0'])


def standalone(eng, launches):
    import torch
    out = {}
    h, w = 140, 250
    for n in (32, 300, 1800):
        maps = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=eng.device)
        prof = torch.zeros((n, h + w), dtype=torch.int32, device=eng.device)
        for _ in range(20):
            eng.border_profile(maps, out=prof)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            eng.border_profile(maps, out=prof)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / launches
        out['%d_maps' % n] = dict(us_per_launch=round(ms * 1e3, 2), bytes_read=n * h * w,
                                  eff_tbs=round(n * h * w / (ms * 1e-3) / 1e12, 4),
                                  frac_of_hbm=round(n * h * w / (ms * 1e-3) / 1e12 / HBM_TBS, 4))
    return out


def last_class(eng, passes):
    import torch
    from retargetvid_amd import synth
    fr = torch.from_numpy(synth.blob_frames(32, 140, 250, seed=0)).to(eng.device)
    cen = torch.zeros((32, 4), dtype=torch.int32, device=eng.device)
    prof = torch.zeros((32, 390), dtype=torch.int32, device=eng.device)
    res = {'flat': [], 'profile': []}
    for _ in range(5):
        eng.saliency(fr, threshold=120, census=cen)
        eng.saliency(fr, threshold=120, census=cen, profile=prof)
    eng.profile_enable('smooth')
    for rep in range(6):                                    # alternating
        for name, p in (('flat', None), ('profile', prof)):
            for _ in range(passes):
                eng.saliency(fr, threshold=120, census=cen, profile=p)
            ms, cnt = eng.profile_read()
            res[name].append(round(ms / cnt * 1e3, 2))
    eng.profile_enable(None)
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(us_per_pass_flat=res['flat'], us_per_pass_profile=res['profile'], median_flat_us=med(res['flat']),
                median_profile_us=med(res['profile']), median_difference_us=round(med(res['profile']) - med(res['flat']), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--passes', type=int, default=50)
    ap.add_argument('--videos', type=int, default=200)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--t-border', type=int, default=90)
    ap.add_argument('--skip-job', action='store_true')
    ap.add_argument('--commit', default=None, help='recorded in the JSON (default: git rev-parse of the tree, if it is one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'border_detection.json'))
    ap.add_argument('--job-dir', default=os.path.join(ROOT, 'build', 'border_job'),
                    help='where the jobs write their result files (build/ is ignored by git)')
    args = ap.parse_args()
    res = {}
    if not args.skip_job:                                   # child processes, before this one opens the GPU
        res['job'] = [job(args.videos, args.repeat, tb, args.job_dir + '_%d' % tb) for tb in (-1, args.t_border, -1, args.t_border)]
    import torch
    from retargetvid_amd import ops
    torch.cuda.set_device(0)
    eng = ops.Engine(device=0)
    res['standalone_140x250'] = standalone(eng, args.launches)
    res['last_class_32_frames_140x250'] = last_class(eng, args.passes)
    eng.close()
    try:
        res['commit'] = args.commit or subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        res['commit'] = None
    res['box'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(line + '\n')


if __name__ == '__main__':
    main()
