"""The last stage of the saliency pass -- pre-softmax map PRE (fp32) -> uint8 map -- as the interval a correct evaluation must
land in, computed in float64 from the PRE it was given.  No network, no convolution: a check against it costs milliseconds.

The device computes, per frame,  u8 = trunc(255 * expf(pre - max pre))  in fp32 (csrc/svc_net.hip: k_quantise, k_quantise_profile);
the reference computes  trunc(exp(log_softmax(pre)) / max * 255)  in fp32 (oracle.unisal_ref.quantise_u8).  The softmax normaliser
cancels, so both round the same real number v* = 255 exp(pre - max); they differ in which roundings they make on the way."""
import numpy as np

U24, U23 = 2.0 ** -24, 2.0 ** -23
UNDERFLOW = 0.5            # below it the map is 0 whatever expf does with a tiny or denormal result


def _vstar(pre32):
    pre = np.asarray(pre32)
    assert pre.dtype == np.float32 and pre.ndim == 2 and np.isfinite(pre).all()
    x = pre.astype(np.float64)
    m = x.max()
    d = x - m                                   # float64: its own rounding, 2^-53 relative, is nothing beside delta
    with np.errstate(under='ignore'):
        return x, m, d, 255.0 * np.exp(d)


def _interval(v, delta):
    with np.errstate(under='ignore'):
        lo = np.clip(np.floor(v * (1.0 - delta)), 0, 255).astype(np.int64)
        hi = np.clip(np.floor(v * (1.0 + delta)), 0, 255).astype(np.int64)
    lo[v < UNDERFLOW] = 0
    hi[v < UNDERFLOW] = 0
    return lo, hi


def map_interval(pre32, ulp_exp=1):
    """One frame's fp32 PRE [h, w] -> (lo, hi, is_max): int64 grey levels lo <= hi and a bool mask, all from float64 arithmetic.

    m = max(pre), d = pre - m, v* = 255 exp(d), delta = 2^-24 |d| + (ulp_exp + 1) 2^-23,
    lo = floor(v* (1 - delta)), hi = floor(v* (1 + delta)), clipped to 0..255; lo = hi = 0 where v* < 0.5; is_max = (pre == m).

    Where delta comes from -- the fp32 roundings of  (uint8_t)(expf(pre - m) * 255.0f):
      * fl(pre - m) is off by at most 2^-24 |d| (half an ulp of the difference); exp turns an absolute error of its argument
        into the same relative error of its value;
      * expf carries the HIP device library's documented bound of 1 ulp (HIP math API, single precision: expf, maximum ulp
        error 1), i.e. 2^-23 relative -- ulp_exp; it changes only to another DOCUMENTED figure;
      * the product by 255 rounds once: 2^-24;
      * one further 2^-24 is slack for the second-order terms of the three factors (1 + e_i);
      * the library is compiled with -ffp-contract=off: the subtraction and the product are not fused with anything.
    Together 2^-24 |d| + ulp_exp 2^-23 + 2 2^-24.  The cast truncates, hence floor on both ends.  Below v* = 0.5 -- long before
    expf's results turn tiny and then denormal (d < -87) -- every admissible value truncates to 0.

    The rules a device map u8 obeys (violations() applies them): u8 in {lo, hi} at every pixel; u8 == 255 wherever is_max, exactly
    -- expf(0) = 1 and 1 * 255 have no rounding -- although the formula gives (254, 255) there; every frame has an is_max pixel;
    behind a threshold t the output is in {0 if a < t else a : a in {lo, hi}}.  A pixel is AMBIGUOUS when lo != hi."""
    x, m, d, v = _vstar(pre32)
    delta = U24 * np.abs(d) + (ulp_exp + 1) * U23
    lo, hi = _interval(v, delta)
    is_max = x == m
    assert is_max.any()
    return lo, hi, is_max


def ref_interval(pre32):
    """The same for the REFERENCE's formulation (oracle.unisal_ref.quantise_u8) -> (lo, hi) with
    delta_ref = 2^-24 (|ls_x| + |ls_max|) + 4 2^-23,  ls = x - logsumexp(x)  (float64).

    Its fp32 roundings: ls_x = fl(log_softmax(x)) is off by 2^-24 |ls_x|, an absolute error that exp turns into a relative one, and
    so is ls_max for the pixel it divides by; exp of each, 1 ulp = 2^-23 twice; the quotient p / max p and the product by 255,
    2^-24 each: 2^-24 (|ls_x| + |ls_max|) + 3 2^-23.  One more 2^-23 covers the second-order terms and the rounding of the
    log-sum itself, which is common to ls_x and ls_max and cancels to first order in the quotient."""
    x, m, d, v = _vstar(pre32)
    with np.errstate(under='ignore'):
        lse = m + np.log(np.exp(d).sum())
    delta = U24 * (np.abs(x - lse) + abs(m - lse)) + 4 * U23
    return _interval(v, delta)


def violations(u8, lo, hi, is_max, thr=0):
    """Bool mask of the pixels of a device map (thresholded at thr: v < thr -> 0) that break a rule of map_interval."""
    u = np.asarray(u8).astype(np.int64)
    cut = lambda a: np.where(a < thr, 0, a)
    bad = (u != cut(lo)) & (u != cut(hi))
    return bad | (is_max & (u != cut(np.full_like(lo, 255))))


def describe(pre32, u8, bad, limit=4):
    """The first offending pixels as (y, x, pre, m, v*, device value) for a failure message or a report."""
    x, m, d, v = _vstar(pre32)
    return [(int(y), int(c), float(x[y, c]), float(m), float(v[y, c]), int(np.asarray(u8)[y, c])) for y, c in np.argwhere(bad)[:limit]]
