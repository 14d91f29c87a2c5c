"""NumPy statement of the four NV12 colours -- BT.601 and BT.709, limited and full range -- for the colour tests (a helper
module, not a conftest): the table of include/svc.h, the rule three of its rows are derived by, and both formulas.

An NV12 frame is laid out as nv12_ref describes.  Every variant has the same arithmetic: 20-bit fixed point, arithmetic
shifts, clamp to 0..255.  Decode, for a pixel's Y and its replicated U V pair:

    yy = max(0, Y - Y0) * CY + (1 << 19),  u = U - 128,  v = V - 128
    R = clamp((yy + CVR v) >> 20)   G = clamp((yy + CVG v + CUG u) >> 20)   B = clamp((yy + CUB u) >> 20)

Encode, for an RGB crop (r, g, b a pixel; sr, sg, sb the sums over a 2 x 2 block):

    Y = clamp((YR r + YG g + YB b + (Y0 << 20) + (1 << 19)) >> 20)
    U = clamp((UR sr + UG sg + UB sb + (128 << 22) + (1 << 21)) >> 22)        V likewise with VR VG VB

The device works in int32; here every intermediate is int64, so that an overflow on the device could not hide behind the same
overflow in the expectation."""
from fractions import Fraction

import numpy as np

MATRICES = ('bt601', 'bt709')
RANGES = ('limited', 'full')
VARIANTS = tuple((m, r) for m in MATRICES for r in RANGES)
DEFAULT = ('bt601', 'limited')
NEW_VARIANTS = tuple(v for v in VARIANTS if v != DEFAULT)
DEC_NAMES = ('Y0', 'CY', 'CVR', 'CVG', 'CUG', 'CUB')
ENC_NAMES = ('YR', 'YG', 'YB', 'UR', 'UG', 'UB', 'VR', 'VG', 'VB')

# (matrix, range) -> (Y0, CY, CVR, CVG, CUG, CUB), (YR, YG, YB, UR, UG, UB, VR, VG, VB): the table of include/svc.h
TABLE = {
    ('bt601', 'limited'): ((16, 1220542, 1673527, -852492, -409993, 2116026),
                           (269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448)),
    ('bt601', 'full'): ((0, 1048576, 1470104, -748826, -360853, 1858077),
                        (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262)),
    ('bt709', 'limited'): ((16, 1220945, 1879825, -558796, -223607, 2215014),
                           (191455, 644068, 65019, -105533, -355018, 460551, 460551, -418321, -42230)),
    ('bt709', 'full'): ((0, 1048576, 1651297, -490864, -196424, 1945738),
                        (222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074)),
}

KR_KB = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)), 'bt709': (Fraction(2126, 10000), Fraction(722, 10000))}


def _round(q):
    """A Fraction times 2^20, rounded half away from zero."""
    q = q * (1 << 20)
    n = (abs(q) * 2 + 1) // 2
    return int(n if q >= 0 else -n)


def derive(matrix, rng):
    """The row of (matrix, rng) from Kr, Kb by the rule of include/svc.h, in exact rational arithmetic.  (BT.601 limited is NOT
    derived this way: it keeps the three-decimal constants OpenCV publishes.)"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    s, c = (Fraction(255, 219), Fraction(255, 224)) if rng == 'limited' else (Fraction(1), Fraction(1))
    y0 = 16 if rng == 'limited' else 0
    dec = (y0, _round(s), _round(2 * (1 - kr) * c), _round(-2 * kr * (1 - kr) * c / kg), _round(-2 * kb * (1 - kb) * c / kg),
           _round(2 * (1 - kb) * c))
    yr, yb = _round(kr / s), _round(kb / s)
    yg = _round(1 / s) - yr - yb                                   # white -> exactly 235 | 255
    ur, ub = _round(-kr / (2 * (1 - kb) * c)), _round(Fraction(1, 2) / c)
    vr, vb = _round(Fraction(1, 2) / c), _round(-kb / (2 * (1 - kr) * c))
    return dec, (yr, yg, yb, ur, -ub - ur, ub, vr, -vr - vb, vb)      # grey -> exactly 128


def variant(colour):
    """None | (matrix, range) | dict(matrix=, range=) -> (matrix, range)."""
    if colour is None:
        return DEFAULT
    if isinstance(colour, dict):
        return (colour.get('matrix', 'bt601'), colour.get('range', 'limited'))
    return tuple(colour)


def yuv_to_rgb_raw(Y, U, V, colour=None):
    """Arrays of Y, U, V (one shape) -> int64 [..., 3]: the three sums BEFORE the shift and the clamp."""
    y0, cy, cvr, cvg, cug, cub = TABLE[variant(colour)][0]
    yy = np.maximum(0, np.asarray(Y).astype(np.int64) - y0) * cy + (1 << 19)
    u = np.asarray(U).astype(np.int64) - 128
    v = np.asarray(V).astype(np.int64) - 128
    return np.stack([yy + cvr * v, yy + cvg * v + cug * u, yy + cub * u], axis=-1)


def yuv_to_rgb(Y, U, V, colour=None):
    """Arrays of Y, U, V (any integer type, one shape) -> uint8 [..., 3] RGB."""
    return np.clip(yuv_to_rgb_raw(Y, U, V, colour) >> 20, 0, 255).astype(np.uint8)


def nv12_to_rgb(frames, h, w, colour=None):
    """uint8 [n, h * 3 / 2, w] (or one frame [h * 3 / 2, w]) -> uint8 [n, h, w, 3] ([h, w, 3])."""
    f = np.asarray(frames)
    single = f.ndim == 2
    if single:
        f = f[None]
    assert f.dtype == np.uint8 and h % 2 == 0 and w % 2 == 0 and h >= 2 and w >= 2 and f.shape[1:] == (h * 3 // 2, w), f.shape
    Y = f[:, :h, :]
    uv = f[:, h:, :].reshape(f.shape[0], h // 2, w // 2, 2)
    U = np.repeat(np.repeat(uv[..., 0], 2, axis=1), 2, axis=2)
    V = np.repeat(np.repeat(uv[..., 1], 2, axis=1), 2, axis=2)
    out = yuv_to_rgb(Y, U, V, colour)
    return out[0] if single else out


def luma_raw(r, g, b, colour=None):
    """int64 sum of the Y formula before the shift (r, g, b: arrays of one shape)."""
    y0 = TABLE[variant(colour)][0][0]
    yr, yg, yb = TABLE[variant(colour)][1][:3]
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    return yr * r + yg * g + yb * b + (y0 << 20) + (1 << 19)


def chroma_raw(sr, sg, sb, colour=None):
    """int64 sums of the U and V formulas before the shift (sr, sg, sb: sums over a 2 x 2 block, 0..1020) -> (u, v)."""
    ur, ug, ub, vr, vg, vb = TABLE[variant(colour)][1][3:]
    sr, sg, sb = (np.asarray(c).astype(np.int64) for c in (sr, sg, sb))
    off = (128 << 22) + (1 << 21)
    return ur * sr + ug * sg + ub * sb + off, vr * sr + vg * sg + vb * sb + off


def rgb_to_nv12(rgb, colour=None):
    """uint8 [n, h, w, 3] (or one crop [h, w, 3]; h, w even) -> uint8 [n, h * 3 / 2, w] ([h * 3 / 2, w])."""
    x = np.asarray(rgb)
    single = x.ndim == 3
    if single:
        x = x[None]
    n, h, w, c = x.shape
    assert x.dtype == np.uint8 and c == 3 and h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0, x.shape
    x = x.astype(np.int64)
    y = luma_raw(x[..., 0], x[..., 1], x[..., 2], colour)
    s = x.reshape(n, h // 2, 2, w // 2, 2, 3).sum(axis=(2, 4))
    u, v = chroma_raw(s[..., 0], s[..., 1], s[..., 2], colour)
    assert 0 <= min(y.min(), u.min(), v.min()) and max(y.max(), u.max(), v.max()) < 2 ** 31
    out = np.empty((n, h * 3 // 2, w), np.uint8)
    out[:, :h] = np.clip(y >> 20, 0, 255)
    out[:, h:, 0::2] = np.clip(u >> 22, 0, 255)
    out[:, h:, 1::2] = np.clip(v >> 22, 0, 255)
    return out[0] if single else out
