"""Inputs of the focus-stability tests (tests/test_focus_host.py, tests/test_gpu_focus.py): the random maps and the four centre kinds
of tests/test_host_native.py's focus test, the battery built from them, and a census of the battery's rows computed from the oracle
(oracle/temporal_ref.py).  NumPy and the oracle only: no GPU, no library."""
import math

import numpy as np

from oracle import temporal_ref as TR

SHAPES = ((35, 62), (140, 250), (250, 140), (249, 249))
MIN_DS = (1, 10)                    # min_d_jump of the best and of the default parameter set


def centres(rng, kind, n, h, w):
    """anywhere (also just outside the image) / integer-valued, with two moves along an axis / a slow random walk / one row"""
    if kind == 0:
        dx, dy = rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)
    elif kind == 1:
        dx, dy = np.round(rng.uniform(0, w, n)), np.round(rng.uniform(0, h, n))
        dx[3], dy[5] = dx[2], dy[4]
    elif kind == 2:
        dx, dy = np.cumsum(rng.randn(n) * 0.7) + w / 2, np.cumsum(rng.randn(n) * 0.4) + h / 2
    else:
        dx, dy = rng.uniform(0, w, n), np.full(n, float(rng.randint(0, h)))
    return [float(v) for v in dx], [float(v) for v in dy]          # Python floats, as the pipeline hands them on


def random_maps(rng, n, h, w):
    maps = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        maps[i] = np.where(rng.rand(h, w) < rng.choice([0.02, 0.2, 0.6]), rng.randint(90, 256, (h, w)), 0)
    return maps


def battery(trials=48, seed=0):
    """-> [(trial, maps uint8 [n, h, w], xy float64 [n, 2])]: shape SHAPES[(trial // 4) % 4], kind trial % 4, n in 7 .. 39."""
    rng = np.random.RandomState(seed)
    out = []
    for trial in range(trials):
        n = rng.randint(7, 40)
        h, w = SHAPES[(trial // 4) % 4]
        maps = random_maps(rng, n, h, w)
        dx, dy = centres(rng, trial % 4, n, h, w)
        out.append((trial, maps, np.stack([dx, dy], 1)))
    return out


def oracle_jumps(maps, xy, min_d):
    """The oracle's jump statistic of every row (row 0: 255), as focus_stability forms them.  The centres go in as Python floats, as
    the pipeline hands them on: a NumPy float64 scalar would promote the oracle's float32 buffer arithmetic to float64."""
    x, y = [float(v) for v in xy[:, 0]], [float(v) for v in xy[:, 1]]
    return [255] + [TR.mean_saliency_on_jump(maps[i], x[i - 1], y[i - 1], x[i], y[i], min_d) for i in range(1, len(x))]


def census(cases, min_ds=MIN_DS):
    """Counts of the rows i >= 1 of every case under every min_d, by what the line walk does with them, from the oracle."""
    c = dict(rows=0, statistic=0, below_min_d=0, m_gt_64=0, m_gt_128=0, m_eq_64=0, m_eq_65=0, one_axis=0, clipped=0)
    for _, maps, xy in cases:
        h, w = maps.shape[1:]
        for min_d in min_ds:
            for i in range(1, len(xy)):
                (p1x, p1y), (p2x, p2y) = xy[i - 1].tolist(), xy[i].tolist()         # Python floats (see oracle_jumps)
                c['rows'] += 1
                if abs(p2x - p1x) < min_d and abs(p2y - p1y) < min_d:
                    c['below_min_d'] += 1
                    continue
                try:
                    pts = TR.points_on_line(p1x, p1y, p2x, p2y, w, h, min_d=min_d)
                except ValueError:                  # NumPy refuses an arange of another length than the buffer's
                    pts = None
                if pts is None or not len(pts):
                    continue
                m = int(math.ceil(max(abs(p2x - p1x), abs(p2y - p1y))))
                c['statistic'] += 1
                c['m_gt_64'] += m > 64
                c['m_gt_128'] += m > 128
                c['m_eq_64'] += m == 64
                c['m_eq_65'] += m == 65
                c['one_axis'] += p1x == p2x or p1y == p2y
                c['clipped'] += len(pts) < m
    return {k: int(v) for k, v in c.items()}
