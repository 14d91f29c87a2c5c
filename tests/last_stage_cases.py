"""Shared by tests/test_last_stage_host.py and tests/test_gpu_last_stage.py: the directed logit fields of the last stage and the
check of one frame's map against the interval of its own pre-softmax map (oracle/last_stage_ref.py)."""
import numpy as np

from oracle import last_stage_ref as L

AMBIGUOUS_CAP = 1e-3          # of a case's pixels: a condition on the case, not a measurement of the device
FIELDS = ('levels1', 'levels3', 'deep', 'negative', 'apart', 'flat', 'tie', 'signed_zero')


def base(H3, W3, n=3):
    """One N(0, 1) base per shape, every frame different."""
    return np.random.RandomState(1000 * H3 + W3).standard_normal((n, H3, W3)).astype(np.float32)


def fields(H3, W3):
    """name -> logits [3, H3, W3]:
    levels1, levels3  the base x1 and x3: most grey levels occupied
    deep              x100: expf underflows and turns denormal; zeros exactly where v* < 0.5, no NaN
    negative          x1 - 5000: the negative branch of the maximum's encoding
    apart             frame offsets +5000, 0, -5000 in one call: a maximum taken from another frame turns a map all 0 or all 255
    flat              constant -3.0: every pixel equal to the maximum
    tie               levels1 with its largest cell copied to a second, distant cell
    signed_zero       nothing above zero, and a block of +0.0 and -0.0 cells wide enough for pre-softmax pixels that are exactly zero"""
    b = base(H3, W3)
    tie = b.copy()
    for f in range(3):
        y, x = np.unravel_index(int(np.argmax(b[f])), (H3, W3))
        tie[f, (y + H3 // 2) % H3, (x + W3 // 2) % W3] = b[f, y, x]
    sz = -np.abs(b) - np.float32(0.25)
    y0, x0 = H3 // 4, W3 // 4
    yy, xx = np.mgrid[0:14, 0:14]
    sz[:, y0:y0 + 14, x0:x0 + 14] = np.where((yy + xx) & 1, np.float32(-0.0), np.float32(0.0))
    out = {'levels1': b, 'levels3': 3 * b, 'deep': 100 * b, 'negative': b - np.float32(5000),
           'apart': b + np.array([5000, 0, -5000], np.float32)[:, None, None], 'flat': np.full_like(b, -3.0), 'tie': tie,
           'signed_zero': sz}
    assert tuple(out) == FIELDS and all(v.dtype == np.float32 and v.shape == b.shape for v in out.values())
    return out


def attribution_logits(n, H3, W3):
    """A full pass of n frames: offsets alternate +5000 and -5000, a different amplitude per frame."""
    b = base(H3, W3, n)
    amp = (1.0 + 0.25 * np.arange(n)).astype(np.float32)
    off = np.where(np.arange(n) & 1, -5000, 5000).astype(np.float32)
    return b * amp[:, None, None] + off[:, None, None]


def add(a, b):
    return {k: a.get(k, 0) + b[k] for k in b}


def check_cap(stats, where):
    """The condition on a CASE (the frames of one call): at most AMBIGUOUS_CAP of its pixels are ambiguous.  The flat field is
    exempt: its pixels are all the maximum up to the smoothing's own rounding, and the exact rule decides at the maximum."""
    assert stats['ambiguous'] <= AMBIGUOUS_CAP * stats['pixels'], (where, 'the case is no test: ambiguous pixels', stats)


def check_frame(pre, u8, where, thr=0):
    """The rules of last_stage_ref.map_interval on one frame -> dict(pixels, ambiguous, took_lo, took_hi).  AMBIGUOUS: lo != hi
    away from the maximum (at the maximum the exact rule decides, whatever the formula gives)."""
    pre = np.ascontiguousarray(pre, np.float32)
    assert np.isfinite(pre).all(), (where, 'PRE is not finite', int((~np.isfinite(pre)).sum()))
    lo, hi, is_max = L.map_interval(pre)
    u = np.asarray(u8).astype(np.int64)
    bad = L.violations(u, lo, hi, is_max, thr)
    assert not bad.any(), (where, 'thr %d' % thr, int(bad.sum()), '(y, x, pre, m, v*, device)', L.describe(pre, u, bad))
    amb = (lo != hi) & ~is_max
    return dict(pixels=int(amb.size), ambiguous=int(amb.sum()), took_lo=int((amb & (u == lo)).sum()), took_hi=int((amb & (u == hi)).sum()))
