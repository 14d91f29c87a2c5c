"""GPU box helper: error of every network tap (HIP vs the FLOAT64 oracle) at the eleven network input sizes, per checkpoint family
and matrix pipe -- the numbers behind the tolerances of tests/test_gpu_parity.py and tests/test_gpu_geometries.py.

Per (checkpoint, pipe, geometry, tap): max and mean |device - float64| / max|float64| over the frames; per (checkpoint, pipe,
geometry): the fraction of u8 pixels one grey level off the fp32 oracle and off the reference model's maps (goldens; on the pixels
they hold: every other row and column for nc / ri at the eight sizes of unisal_golden5.npz).  Frames and
checkpoints are those of tests/test_gpu_geometries.py.

  python tools/net_error_report.py [--ck carrier,nc,ri,tl,tl2] [--f32 tl] [--geoms 16x9,1x1,...] [--out report.md]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from retargetvid_amd import ops                                                 # noqa: E402
import test_gpu_geometries as G                                                 # noqa: E402

TAPS = [key for key, _, _, _ in G._TAPS] + ['pre']


def measure(ck, pipe, geoms):
    eng = G._engine(G._checkpoint(ck), pipe)
    rows = []
    try:
        for gname in geoms:
            h, w = G.ELEVEN[gname]
            NH, NW = G.NET_SIZES[gname]
            fr, gold, ref32, _, taps64 = G._oracle(ck, gname)
            maps = eng.saliency(torch.from_numpy(fr).cuda()).cpu().numpy()
            err = {k: [0.0, 0.0] for k in TAPS}
            for i in range(len(fr)):
                for key, tap, div, ch in G._TAPS + (('pre', 'TAP_PRE', None, None),):
                    got = eng.tap(getattr(ops, tap), i, (NH // div, NW // div, ch) if div else (h, w))
                    if key == 'feat_1x':
                        got = got[:, :, :1280]
                    ref = taps64[i][key]
                    d = np.abs(got.astype(np.float64) - ref) / np.abs(ref).max()
                    err[key][0] = max(err[key][0], float(d.max()))
                    err[key][1] = max(err[key][1], float(d.mean()))
            flips = [float((maps != ref32).mean()),
                     None if gold is None else float(np.mean([(maps[i][idx] != r8).mean() for i, (r8, idx) in enumerate(gold)]))]
            rows.append((gname, err, flips))
            print(ck, pipe, gname, ' '.join('%s %.1e/%.1e' % (k, *err[k]) for k in TAPS),
                  'u8 flips %.4f%% / %s' % (100 * flips[0], '-' if flips[1] is None else '%.4f%%' % (100 * flips[1])), flush=True)
    finally:
        eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ck', default='carrier,nc,ri,tl,tl2')
    ap.add_argument('--f32', default='tl', help='checkpoints also run on the fp32 matrix pipe (SVC_MX=f32)')
    ap.add_argument('--geoms', default=','.join(G.ELEVEN))
    ap.add_argument('--out', default=None, help='also write the table as markdown to this file')
    a = ap.parse_args()
    geoms = a.geoms.split(',')
    runs = [(ck, 'bf16x6') for ck in a.ck.split(',')] + [(ck, 'f32') for ck in a.f32.split(',') if ck]
    lines = ['| checkpoint | pipe | map | network | ' + ' | '.join('%s max / mean' % k for k in TAPS) +
             ' | u8 flips vs fp32 oracle | u8 flips vs reference |',
             '|' + '---|' * (4 + len(TAPS) + 2)]
    for ck, pipe in runs:
        for gname, err, flips in measure(ck, pipe, geoms):
            h, w = G.ELEVEN[gname]
            NH, NW = G.NET_SIZES[gname]
            lines.append('| %s | %s | %dx%d | %dx%d | ' % (ck, pipe, h, w, NH, NW) +
                         ' | '.join('%.1e / %.1e' % tuple(err[k]) for k in TAPS) +
                         ' | %.3f %% | %s |' % (100 * flips[0], '-' if flips[1] is None else '%.3f %%' % (100 * flips[1])))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
