"""NumPy statement of the sub-pixel windows of svc_render_windows_q8 (include/svc.h), for the sub-pixel tests (a helper module, not
a conftest).  Built on oracle.cv_ref's INTER_LINEAR table (_linear_coeffs: offsets, 11-bit weights, xmax) and its two-stage blend,
and on nv12_ref / colour_ref / nv12_out_ref for the conversions on either side; never on the code under test.

The top-left corner of frame f's bw x bh window is given in 1/256 pixel.  X = clamp(origin_x, 0, (w - bw) * 256), xi = X >> 8,
xf = X & 255; Y, yi, yf likewise.  With T the table of (bh, bw) -> (oh, ow):

    columns  sx, a0, a1 = T (sx clamped into the window, the fraction zero where it was), right tap min(sx + 1, bw - 1), a plain
             copy from xmax on.  xf > 0:  p = sx * 2048 + a1 + 8 * xf,  sx' = p >> 11,  a1' = p & 2047,  a0' = 2048 - a1',
             taps xi + sx' and xi + sx' + 1, both weighted
    rows     y0 = clip(sy, 0, bh - 1), y1 = clip(sy + 1, 0, bh - 1), b0, b1 = T.  yf > 0:  q = y0 * 2048 + (b1 if y1 > y0 else 0)
             + 8 * yf,  sy' = q >> 11,  b1' = q & 2047,  b0' = 2048 - b1',  rows yi + sy' and yi + sy' + 1
    value    h = t0 * a0 + t1 * a1 per row (t0 * 2048 for a plain copy),
             clip((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0, 255)

A zero phase leaves the table's taps and weights as they are.  Every intermediate is int64."""
import numpy as np

import colour_ref
import nv12_out_ref
import nv12_ref
from oracle import cv_ref

ONE = cv_ref.COEF_SCALE          # 2048
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def clamp_origins(origins_q8, h, w, bh, bw):
    """int [n, 2] (x, y) in 1/256 px -> (xi, xf, yi, yf), int64 [n] each, of the clamped origins."""
    o = np.asarray(origins_q8, np.int64).reshape(-1, 2)
    X = np.clip(o[:, 0], 0, (w - bw) * 256)
    Y = np.clip(o[:, 1], 0, (h - bh) * 256)
    return X >> 8, X & 255, Y >> 8, Y & 255


def column_taps(bw, ow, xf):
    """The two window columns of every output column and their weights at the phases xf [n] -> s0, s1, a0, a1 (int64 [n, ow]) and
    copy (bool [n, ow]: only s0 counts, at full weight)."""
    xofs, alpha, xmax = cv_ref._linear_coeffs(bw, ow, float(bw) / ow, True)
    n = len(xf)
    s0 = np.broadcast_to(xofs, (n, ow)).copy()
    s1 = np.minimum(s0 + 1, bw - 1)
    a0 = np.broadcast_to(alpha[:, 0], (n, ow)).copy()
    a1 = np.broadcast_to(alpha[:, 1], (n, ow)).copy()
    copy = np.broadcast_to(np.arange(ow) >= xmax, (n, ow)).copy()
    m = np.asarray(xf) > 0
    p = s0[m] * ONE + a1[m] + 8 * np.asarray(xf, np.int64)[m, None]
    s0[m], a1[m] = p >> 11, p & (ONE - 1)
    s1[m], a0[m], copy[m] = s0[m] + 1, ONE - a1[m], False
    return s0, s1, a0, a1, copy


def row_taps(bh, oh, yf):
    """The same for the rows -> r0, r1, b0, b1 (int64 [n, oh])."""
    yofs, beta, _ = cv_ref._linear_coeffs(bh, oh, float(bh) / oh, False)
    n = len(yf)
    r0 = np.broadcast_to(np.clip(yofs, 0, bh - 1), (n, oh)).copy()
    r1 = np.broadcast_to(np.clip(yofs + 1, 0, bh - 1), (n, oh)).copy()
    b0 = np.broadcast_to(beta[:, 0], (n, oh)).copy()
    b1 = np.broadcast_to(beta[:, 1], (n, oh)).copy()
    m = np.asarray(yf) > 0
    q = r0[m] * ONE + np.where(r1[m] > r0[m], b1[m], 0) + 8 * np.asarray(yf, np.int64)[m, None]
    r0[m], b1[m] = q >> 11, q & (ONE - 1)
    r1[m], b0[m] = r0[m] + 1, ONE - b1[m]
    return r0, r1, b0, b1


def windows_rgb(frames_rgb, origins_q8, bw, bh, oh, ow):
    """uint8 [n, h, w, 3] RGB frames and their origins -> the RGB crops uint8 [n, oh, ow, 3]."""
    fr = np.asarray(frames_rgb)
    n, h, w, _ = fr.shape
    assert fr.dtype == np.uint8 and 1 <= bw <= w and 1 <= bh <= h
    xi, xf, yi, yf = clamp_origins(origins_q8, h, w, bh, bw)
    assert len(xi) == n
    s0, s1, a0, a1, copy = column_taps(bw, ow, xf)
    r0, r1, b0, b1 = row_taps(bh, oh, yf)
    c0, c1 = xi[:, None] + s0, xi[:, None] + s1
    y0, y1 = yi[:, None] + r0, yi[:, None] + r1
    assert c0.min() >= 0 and c1.max() <= w - 1 and y0.min() >= 0 and y1.max() <= h - 1       # every tap is a pixel of the frame
    src = fr.astype(np.int64)
    f = np.arange(n)[:, None, None]

    def hrow(y):            # the horizontal pass of frame rows y [n, oh] -> int64 [n, oh, ow, 3]
        t0, t1 = src[f, y[:, :, None], c0[:, None, :]], src[f, y[:, :, None], c1[:, None, :]]
        both = t0 * a0[:, None, :, None] + t1 * a1[:, None, :, None]
        return np.where(copy[:, None, :, None], t0 * ONE, both)
    h0, h1 = hrow(y0), hrow(y1)
    out = (((b0[:, :, None, None] * (h0 >> 4)) >> 16) + ((b1[:, :, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def to_rgb(frames, pix_fmt, h, w, colour=None):
    """Packed frames of `pix_fmt` -> uint8 [n, h, w, 3] RGB (nv12: decoded in `colour`, None = BT.601 limited)."""
    if pix_fmt == 'rgb24':
        return np.asarray(frames)
    return nv12_ref.nv12_to_rgb(frames, h, w) if colour is None else colour_ref.nv12_to_rgb(frames, h, w, colour)


def deliver(crops_rgb, out_fmt='rgb24', bgr=False, out_colour=None):
    """RGB crops uint8 [n, oh, ow, 3] -> what the renderer writes: RGB, BGR, or NV12 frames uint8 [n, oh * 3 / 2, ow]."""
    if out_fmt == 'nv12':
        return nv12_out_ref.rgb_to_nv12_fixed(crops_rgb) if out_colour is None else colour_ref.rgb_to_nv12(crops_rgb, out_colour)
    return np.ascontiguousarray(crops_rgb[..., ::-1]) if bgr else crops_rgb


def render_windows(frames, origins_q8, bw, bh, oh, ow, h, w, pix_fmt='rgb24', out_fmt='rgb24', bgr=False, colour=None, out_colour=None):
    """The packed output of svc_render_windows_q8 on packed frames."""
    return deliver(windows_rgb(to_rgb(frames, pix_fmt, h, w, colour), origins_q8, bw, bh, oh, ow), out_fmt, bgr, out_colour)
