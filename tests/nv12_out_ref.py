"""NumPy statement of the renderer's NV12 output, for the NV12-output tests (a helper module, not a conftest).

The output frame of an RGB crop C [oh, ow, 3] (oh, ow even, >= 2) is uint8 [oh * 3 / 2, ow] in the layout nv12_ref describes:
BT.601 limited range in 20-bit fixed point, arithmetic shifts, the chroma from the SUM of each 2 x 2 block (include/svc.h):

    Y[y][x] = (269484 r + 528482 g + 102760 b + (16 << 20) + (1 << 19)) >> 20
    U[j][i] = (-155188 sr - 305135 sg + 460324 sb + (128 << 22) + (1 << 21)) >> 22
    V[j][i] = ( 460324 sr - 385875 sg -  74448 sb + (128 << 22) + (1 << 21)) >> 22

The device works in int32 (the largest intermediate is 1.01e9); here the intermediates are int64, so that an overflow on the
device could not hide behind the same overflow in the expectation.  Nothing is clamped: Y lands in 16..235, U and V in 16..240."""
import numpy as np

Y_COEF = (269484, 528482, 102760)
U_COEF = (-155188, -305135, 460324)
V_COEF = (460324, -385875, -74448)


def rgb_to_nv12_fixed(rgb):
    """uint8 [n, h, w, 3] (or one crop [h, w, 3]; h, w even) -> uint8 [n, h * 3 / 2, w] ([h * 3 / 2, w])."""
    x = np.asarray(rgb)
    single = x.ndim == 3
    if single:
        x = x[None]
    n, h, w, c = x.shape
    assert x.dtype == np.uint8 and c == 3 and h >= 2 and w >= 2 and h % 2 == 0 and w % 2 == 0, x.shape
    x = x.astype(np.int64)
    y = (x * np.array(Y_COEF, np.int64)).sum(-1) + (16 << 20) + (1 << 19)
    s = x.reshape(n, h // 2, 2, w // 2, 2, 3).sum(axis=(2, 4))
    u = (s * np.array(U_COEF, np.int64)).sum(-1) + (128 << 22) + (1 << 21)
    v = (s * np.array(V_COEF, np.int64)).sum(-1) + (128 << 22) + (1 << 21)
    assert 0 <= min(y.min(), u.min(), v.min()) and max(y.max(), u.max(), v.max()) < 2 ** 31
    y, u, v = y >> 20, u >> 22, v >> 22
    assert y.max() <= 255 and u.max() <= 255 and v.max() <= 255       # (an astype below would wrap silently)
    out = np.empty((n, h * 3 // 2, w), np.uint8)
    out[:, :h] = y
    out[:, h:, 0::2] = u
    out[:, h:, 1::2] = v
    return out[0] if single else out


def every_rgb_triple_frame():
    """One 4096 x 4096 RGB frame that holds every triple once: pixel (y, x) has r = y & 255, g = x & 255,
    b = ((y >> 8) << 4) | (x >> 8)."""
    y, x = np.meshgrid(np.arange(4096), np.arange(4096), indexing='ij')
    return np.stack([y & 255, x & 255, ((y >> 8) << 4) | (x >> 8)], -1).astype(np.uint8)
