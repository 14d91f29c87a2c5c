"""NumPy statement of the NV12 input format and its conversion to RGB, for the NV12 tests (a helper module, not a conftest).

An NV12 frame of a h x w picture (h, w even, >= 2) is uint8 [h * 3 / 2, w]: rows 0 .. h-1 are luma Y; row h + j holds the
chroma of picture rows 2j, 2j+1 as interleaved pairs U(j,0) V(j,0) U(j,1) V(j,1) ...  Pixel (y, x) uses Y[y][x] and the pair
(y >> 1, x >> 1) (chroma replicated, not interpolated).  RGB is BT.601 limited range in 20-bit fixed point, all in int32
(largest magnitude 5.7e8), >> arithmetic -- the constants OpenCV publishes for COLOR_YUV2RGB_NV12:

    yy = max(0, Y - 16) * 1220542          u = U - 128        v = V - 128
    R = clamp((yy + (1 << 19) + 1673527 * v) >> 20, 0, 255)
    G = clamp((yy + (1 << 19) -  852492 * v - 409993 * u) >> 20, 0, 255)
    B = clamp((yy + (1 << 19) + 2116026 * u) >> 20, 0, 255)

nv12_to_rgb is what every expected value of the tests comes from; rgb_to_nv12 (float BT.601 forward, 2x2 chroma mean) only
makes structured NV12 inputs out of the synthetic RGB videos."""
import numpy as np

SHIFT = 20
CY, CVR, CVG, CUG, CUB = 1220542, 1673527, -852492, -409993, 2116026


def yuv_to_rgb(Y, U, V):
    """Arrays of Y, U, V (any integer type, one shape) -> uint8 [..., 3] RGB by the fixed-point formula above."""
    yy = np.maximum(0, np.asarray(Y).astype(np.int32) - 16) * np.int32(CY) + np.int32(1 << (SHIFT - 1))
    u = np.asarray(U).astype(np.int32) - 128
    v = np.asarray(V).astype(np.int32) - 128
    r = (yy + np.int32(CVR) * v) >> SHIFT
    g = (yy + np.int32(CVG) * v + np.int32(CUG) * u) >> SHIFT
    b = (yy + np.int32(CUB) * u) >> SHIFT
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def yuv_to_rgb_float(Y, U, V):
    """The same conversion in float64, unrounded and unclamped except for the luma floor the format defines (Y < 16 is black level):
    BT.601 limited range, R = 1.164383 (Y - 16) + 1.596027 (V - 128) etc. with the exact rational coefficients."""
    y = np.maximum(0.0, np.asarray(Y, np.float64) - 16.0) * (255.0 / 219.0)
    u = np.asarray(U, np.float64) - 128.0
    v = np.asarray(V, np.float64) - 128.0
    kr, kb = 0.299, 0.114
    kg = 1.0 - kr - kb
    s = 255.0 / 224.0
    r = y + 2.0 * (1.0 - kr) * s * v
    g = y - 2.0 * kr * (1.0 - kr) / kg * s * v - 2.0 * kb * (1.0 - kb) / kg * s * u
    b = y + 2.0 * (1.0 - kb) * s * u
    return np.stack([r, g, b], axis=-1)


def nv12_to_rgb(frames, h, w):
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
    out = yuv_to_rgb(Y, U, V)
    return out[0] if single else out


def rgb_to_nv12(rgb):
    """uint8 [n, h, w, 3] (h, w even) -> uint8 [n, h * 3 / 2, w]: float BT.601 limited-range forward transform, chroma = the
    mean of each 2 x 2 block.  Only for MAKING structured inputs: nothing is expected to survive the round trip."""
    x = np.asarray(rgb, np.float64)
    n, h, w, _ = x.shape
    assert h % 2 == 0 and w % 2 == 0
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    out = np.empty((n, h * 3 // 2, w), np.uint8)
    out[:, :h] = np.clip(np.rint(y), 0, 255)
    sub = lambda c: c.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    out[:, h:, 0::2] = np.clip(np.rint(sub(u)), 0, 255)
    out[:, h:, 1::2] = np.clip(np.rint(sub(v)), 0, 255)
    return out


def all_triples_frame():
    """One 4096 x 4096 NV12 frame [6144, 4096] that holds every (Y, U, V) triple: the chroma pair of 2 x 2 block (j, i) is
    (U, V) = (j & 255, i & 255) ... every pair occurs in 64 blocks (j >> 8, i >> 8), and block number k = 8 (j >> 8) + (i >> 8)
    holds the four luma values 4 k .. 4 k + 3."""
    h = w = 4096
    f = np.empty((h * 3 // 2, w), np.uint8)
    j, i = np.meshgrid(np.arange(h // 2), np.arange(w // 2), indexing='ij')
    f[h:, 0::2] = j & 255
    f[h:, 1::2] = i & 255
    k = 8 * (j >> 8) + (i >> 8)
    for dy in range(2):
        for dx in range(2):
            f[dy:h:2, dx::2] = 4 * k + 2 * dy + dx
    return f
