"""tests/golden/border_golden.npz: the reference's OWN sc_border_detection (smartVidCrop.py:842-924) and sc_compute_bb
(:979-1048) run on seeded map stacks, in the BUILD CONTAINER ONLY: the reference module is imported under stub modules for
what it pulls in at import time and never uses here (cv2, ffmpeg, hdbscan, imutils, tensorflow, the two network handlers,
matplotlib ...).  Nothing at test, bench or smoke time imports this file, and the fixture holds data only:

  meta     int32 [N, 6]   h_process, w_process, h_orig, w_orig, t_border, offset of the case's profile in `profiles`
  profiles uint8 [sum h+w] per case: max over time and x of the stack per row (f_col, h values), then max over time and y
                          per column (f_row, w values) -- what the device hands sc_border_detection
  borders  int32 [N, 4]   the reference's border_t, border_b, border_l, border_r
  kind     str   [N]      what the stack looked like
  box_case int32 [M]      case index of every box record;  box_ratio str [M];  box_xy float64 [M, FC, 2] smoothed centres in
                          process pixels (dxs, dys);  boxes int32 [M, FC, 4], fbb int32 [M, 2] (fbb_w, fbb_h): the reference's
                          sc_compute_bb under that case's borders (after its own sc_calc_dest_size)

Run from the repo root:  python tools/make_golden_border.py <directory of the reference's smartVidCrop.py>"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ref_import_svc import load_reference  # noqa: E402  (the stubbed import of the reference: tools/ref_import_svc.py)

FC = 16


# process size, original size: the ratios 360/140, 640/250, 1080/141, 2160/250, 480/166 ... are not integers, so the float order
# of step 4 (int((ho / h) * t)) matters
SIZES = [(140, 250, 360, 640), (250, 140, 640, 360), (166, 250, 480, 720), (141, 250, 1080, 1920), (250, 140, 2160, 1216),
         (140, 250, 1080, 1920), (140, 250, 2160, 3840), (250, 166, 1000, 664)]
KINDS = ['letterbox', 'pillarbox', 'both', 'top_only', 'bottom_only', 'left_only', 'right_only', 'nothing_above', 't0', 't254',
         't255', 'single_pixel', 'noisy_bars', 'no_bars', 'wide_bars', 'dim_picture']


def make_stack(rng, kind, h, w, n=3):
    """-> (stack [h, w, n] u8, t_border)"""
    tb = int(rng.randint(3, 40))
    sm = rng.randint(tb + 1, 256, (h, w, n)).astype(np.uint8)
    sm[rng.rand(h, w, n) < 0.5] = 0                      # bright pixels are sparse: a row can be dark in one map, bright in another
    t, b = int(rng.randint(1, h // 3)), int(rng.randint(1, h // 3))
    l, r = int(rng.randint(1, w // 3)), int(rng.randint(1, w // 3))
    dark = lambda shape: rng.randint(0, tb + 1, shape).astype(np.uint8)        # noqa: E731  (values up to t_border itself: not above it)
    if kind in ('letterbox', 'both', 'top_only', 'noisy_bars'):
        sm[:t] = dark((t, w, n))
    if kind in ('letterbox', 'both', 'bottom_only', 'noisy_bars'):
        sm[h - b:] = dark((b, w, n))
    if kind in ('pillarbox', 'both', 'left_only'):
        sm[:, :l] = dark((h, l, n))
    if kind in ('pillarbox', 'both', 'right_only'):
        sm[:, w - r:] = dark((h, r, n))
    if kind == 'noisy_bars':                             # one pixel above the threshold inside the top bar, in one map only
        sm[int(rng.randint(0, t)), int(rng.randint(0, w)), int(rng.randint(0, n))] = tb + 1
    if kind == 'nothing_above':
        sm = dark((h, w, n))
    if kind == 't0':
        tb = 0
        sm[:t] = 0
        sm[:, w - r:] = 0
    if kind == 't254':
        tb = 254
        sm = rng.randint(0, 255, (h, w, n)).astype(np.uint8)
        sm[int(rng.randint(0, h)), int(rng.randint(0, w)), 0] = 255
        sm[int(rng.randint(0, h)), int(rng.randint(0, w)), n - 1] = 255
    if kind == 't255':
        tb = 255
        sm = rng.randint(0, 256, (h, w, n)).astype(np.uint8)
    if kind == 'single_pixel':
        sm = dark((h, w, n))
        sm[int(rng.randint(0, h)), int(rng.randint(0, w)), int(rng.randint(0, n))] = 255
    if kind == 'wide_bars':                              # wider than the 45 % cap on both axes
        sm[:int(h * 0.48)] = 0
        sm[:, w - int(w * 0.47):] = 0
    if kind == 'dim_picture':                            # picture barely above the threshold, bars exactly at it
        sm = np.full((h, w, n), tb + 1, np.uint8)
        sm[:t] = tb
        sm[:, :l] = tb
    return sm, tb


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    rng = np.random.RandomState(20)
    meta, profs, borders, kinds = [], [], [], []
    box_case, box_ratio, box_xy, boxes, fbb = [], [], [], [], []
    off = 0
    N = 240
    for i in range(N):
        h, w, ho, wo = SIZES[i % len(SIZES)]
        kind = KINDS[(i // len(SIZES) + i) % len(KINDS)]
        sm, tb = make_stack(rng, kind, h, w)
        VD = dict(h_process=h, w_process=w, h_orig=ho, w_orig=wo, smaps=sm)
        CP = ref.sc_init_crop_params()
        CP['t_border'] = tb
        with contextlib.redirect_stdout(io.StringIO()):
            VD = ref.sc_border_detection(CP, VD)
        brd = [int(VD[k]) for k in ('border_t', 'border_b', 'border_l', 'border_r')]
        M = sm.max(2)
        prof = np.concatenate([M.max(1), M.max(0)]).astype(np.uint8)
        meta.append((h, w, ho, wo, tb, off))
        off += prof.size
        profs.append(prof)
        borders.append(brd)
        kinds.append(kind)
        if i % 3 == 0 and any(brd):
            ratios = ['1:3', '3:1'] + (['9:16'] if (ho, wo) == (1080, 1920) else [])
            xy = np.stack([rng.uniform(-5, w + 5, FC), rng.uniform(-5, h + 5, FC)], 1)       # (smoothing can overshoot the map)
            xy[:4] = [(0, 0), (w - 1, h - 1), (w / 2.0, h / 2.0), (w - 1, 0)]
            for ratio in ratios:
                V = dict(VD, fc=FC, dxs=xy[:, 0].tolist(), dys=xy[:, 1].tolist())
                cp = dict(CP, out_ratio=ratio)
                with contextlib.redirect_stdout(io.StringIO()):
                    V = ref.sc_calc_dest_size(V, cp, verbose=False)
                    V = ref.sc_compute_bb(V, cp)
                box_case.append(i)
                box_ratio.append(ratio)
                box_xy.append(xy)
                boxes.append(np.asarray(V['bbs'], np.int64))
                fbb.append((int(V['fbb_w']), int(V['fbb_h'])))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'border_golden.npz')
    np.savez_compressed(out, meta=np.asarray(meta, np.int32), profiles=np.concatenate(profs), borders=np.asarray(borders, np.int32),
                        kind=np.asarray(kinds), box_case=np.asarray(box_case, np.int32), box_ratio=np.asarray(box_ratio),
                        box_xy=np.asarray(box_xy, np.float64), boxes=np.asarray(boxes, np.int32), fbb=np.asarray(fbb, np.int32))
    print('%s: %d cases (%d with non-zero borders), %d box records over %d cases, %d bytes'
          % (out, N, sum(any(b) for b in borders), len(boxes), len(set(box_case)), os.path.getsize(out)))


if __name__ == '__main__':
    main()
