"""No GPU: the NV12 conversion the device kernels implement (tests/nv12_ref.py, the fixed-point BT.601 formula) against a
float64 evaluation on every (Y, U, V) triple, and the host-side validation of an NV12 video dict."""
import numpy as np
import pytest

import nv12_ref
from retargetvid_amd import ops, render, smartVidCrop as S
from retargetvid_amd.frames import FrameSource


def test_fixed_point_conversion_against_float64_on_all_triples():
    """All 2^24 triples, one Y plane at a time: every channel within ONE grey level of the rounded float64 BT.601 value (the
    fixed-point constants are the float coefficients rounded to 20 bits, the >> 20 rounds to nearest) and within 0.7 of the
    unrounded one."""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    worst_r, worst_f, differ = 0, 0.0, np.zeros(3)
    for y in range(256):
        Y = np.full_like(U, y)
        got = nv12_ref.yuv_to_rgb(Y, U, V).astype(np.int64)
        ref = nv12_ref.yuv_to_rgb_float(Y, U, V)
        ref_u8 = np.clip(np.rint(ref), 0, 255).astype(np.int64)
        d = np.abs(got - ref_u8)
        worst_r = max(worst_r, int(d.max()))
        worst_f = max(worst_f, float(np.abs(got - np.clip(ref, 0, 255)).max()))
        differ += (d > 0).reshape(-1, 3).sum(0)
    print('max |fixed - rint(float64)| =', worst_r, ' max |fixed - float64| = %.4f' % worst_f,
          ' share of triples that differ (R, G, B) =', (differ / 2.0 ** 24).round(4).tolist())
    assert worst_r <= 1
    assert worst_f <= 0.70


def test_black_white_and_clamps():
    c = lambda y, u, v: nv12_ref.yuv_to_rgb(np.array([y]), np.array([u]), np.array([v]))[0].tolist()
    assert c(16, 128, 128) == [0, 0, 0]
    assert c(235, 128, 128) == [255, 255, 255]
    for y in range(0, 16):                                   # below black level: the luma term is floored at 0
        assert c(y, 128, 128) == [0, 0, 0]
        assert c(y, 200, 90) == c(16, 200, 90)
    for y in range(236, 256):                                # above white level: the channels saturate
        assert c(y, 128, 128) == [255, 255, 255]
    # the extremes of the chroma terms, evaluated by hand from the formula (clamped at both ends)
    assert c(16, 0, 0) == [0, 154, 0] and c(16, 255, 255) == [203, 0, 255] and c(255, 255, 255) == [255, 125, 255]
    assert c(128, 0, 255) == [255, 77, 0] and c(128, 255, 0) == [0, 185, 255]
    assert c(81, 90, 240) == [254, 0, 0] and c(145, 54, 34) == [0, 255, 1]       # BT.601 red and green


def test_nv12_frame_layout():
    """nv12_to_rgb reads the layout of the specification: luma rows, then interleaved U V rows, one pair per 2 x 2 pixels."""
    h, w = 4, 6
    f = np.zeros((1, 6, 6), np.uint8)
    f[0, :4] = 100
    f[0, 2, 3] = 180                                         # one brighter pixel
    f[0, 4:] = 128
    f[0, 5, 2:4] = (90, 240)                                 # the pair of picture rows 2-3, columns 2-3
    rgb = nv12_ref.nv12_to_rgb(f, h, w)
    grey = nv12_ref.yuv_to_rgb(np.array([100]), np.array([128]), np.array([128]))[0]
    tint = nv12_ref.yuv_to_rgb(np.array([100, 180]), np.array([90, 90]), np.array([240, 240]))
    exp = np.broadcast_to(grey, (4, 6, 3)).copy()
    exp[2:4, 2:4] = tint[0]
    exp[2, 3] = tint[1]
    assert np.array_equal(rgb[0], exp)
    assert np.array_equal(nv12_ref.nv12_to_rgb(f[0], h, w), exp)
    full = nv12_ref.all_triples_frame()
    Y, UV = full[:4096].reshape(2048, 2, 2048, 2), full[4096:].reshape(2048, 2048, 2)
    key = (Y.astype(np.int64) << 16) | (UV[:, None, :, None, 0].astype(np.int64) << 8) | UV[:, None, :, None, 1]
    assert np.unique(key).size == 1 << 24                     # every (Y, U, V) triple occurs


def _video(n=12, h=36, w=64, **kw):
    v = dict(fr=30.0, frame_count=n, w=w, h=h, frames=np.zeros((n, h * 3 // 2, w), np.uint8), trans_inds=[0, n], pix_fmt='nv12')
    v.update(kw)
    return v


def test_plan_video_validates_the_format_without_a_gpu():
    CP = S.sc_init_crop_params()
    plan = S.plan_video(_video(), CP)
    assert plan['source'].pix_fmt == 'nv12' and (plan['h'], plan['w']) == (36, 64) and plan['n_frames'] == 12
    rgb = dict(_video(), frames=np.zeros((12, 36, 64, 3), np.uint8))
    del rgb['pix_fmt']
    assert S.plan_video(rgb, CP)['source'].pix_fmt == 'rgb24'
    assert S.plan_video(dict(rgb, pix_fmt='rgb24'), CP)['source'].pix_fmt == 'rgb24'
    with pytest.raises(ValueError, match='pix_fmt'):
        S.plan_video(_video(pix_fmt='yuv420p'), CP)
    with pytest.raises(ValueError, match='even'):
        S.plan_video(_video(w=63, frames=np.zeros((12, 54, 63), np.uint8)), CP)
    with pytest.raises(ValueError, match='even'):
        S.plan_video(_video(h=35, frames=np.zeros((12, 52, 64), np.uint8)), CP)
    with pytest.raises(ValueError, match='nv12 frames'):       # RGB frames under an NV12 label
        S.plan_video(_video(frames=np.zeros((12, 36, 64, 3), np.uint8)), CP)
    with pytest.raises(ValueError, match='nv12 frames'):       # the luma plane alone
        S.plan_video(_video(frames=np.zeros((12, 36, 64), np.uint8)), CP)
    with pytest.raises(ValueError, match='nv12 frames'):       # another picture size
        S.plan_video(_video(frames=np.zeros((12, 54, 96), np.uint8)), CP)
    # the error comes before shot detection too (no trans_inds: a shot network would have to run on the device)
    with pytest.raises(ValueError, match='nv12 frames'):
        S.plan_video(_video(frames=np.zeros((12, 36, 64), np.uint8), trans_inds=None), CP, shot_net=object())


def test_render_video_validates_the_format_without_a_gpu():
    VD = dict(fc=3, bbs_np=np.array([[0, 0, 10, 36]] * 3, np.int64))
    good = _video(3)
    for bad in (dict(good, pix_fmt='p010'), dict(good, w=63), dict(good, h=35), dict(good, frames=np.zeros((3, 36, 64, 3), np.uint8)),
                dict(good, frames=np.zeros((3, 54, 62), np.uint8))):
        with pytest.raises(ValueError):
            render.render_video(bad, VD, engine=None)          # engine None: a device engine would be built after the checks
    with pytest.raises(ValueError):                            # a bare container takes pix_fmt=; its shape must be an NV12 one
        render.render_video(np.zeros((3, 55, 64), np.uint8), VD, engine=None, pix_fmt='nv12')
    with pytest.raises(ValueError):
        render.render_video(np.zeros((3, 54, 64), np.uint8), VD, engine=None, pix_fmt='nv21')
    with pytest.raises(ValueError, match='outside'):           # the window is checked against the PICTURE, not the container's rows
        render.render_video(good, dict(fc=3, bbs_np=np.array([[0, 0, 10, 40]] * 3, np.int64)), engine=None)
    nhwf = lambda src: (src.n, src.h, src.w, src.pix_fmt)
    assert nhwf(FrameSource.of(good)) == (3, 36, 64, 'nv12')
    assert nhwf(FrameSource.of(np.zeros((3, 54, 64), np.uint8), 'nv12')) == (3, 36, 64, 'nv12')
    assert nhwf(FrameSource.of(np.zeros((3, 36, 64, 3), np.uint8))) == (3, 36, 64, 'rgb24')


def test_frame_shapes():
    assert ops.frame_shape('rgb24', 360, 640) == (360, 640, 3) and ops.frame_shape('nv12', 360, 640) == (540, 640)
    assert ops.picture_size(np.zeros((5, 540, 640), np.uint8), 'nv12') == (5, 360, 640)
    assert ops.picture_size(np.zeros((5, 3, 2), np.uint8), 'nv12') == (5, 2, 2)
    assert ops.picture_size(np.zeros((5, 360, 640, 3), np.uint8), 'rgb24') == (5, 360, 640)
    for bad in ((5, 541, 640), (5, 540, 641), (5, 540, 640, 3), (5, 0, 4)):
        with pytest.raises(ValueError):
            ops.picture_size(np.zeros(bad, np.uint8), 'nv12')
    with pytest.raises(ValueError):
        ops.picture_size(np.zeros((5, 540, 640), np.uint8), 'rgb24')
    for h, w in ((35, 64), (36, 63), (0, 64)):
        with pytest.raises(ValueError):
            ops.frame_shape('nv12', h, w)
    with pytest.raises(ValueError):
        ops.frame_shape('yuv420p', 36, 64)
