"""Sub-pixel crop windows on the host (no GPU): the oracle tests/subpixel_ref.py against itself and against oracle.cv_ref; the origins
sc_compute_bb keeps in VD['bbs_q8']; the Python doors; svc_render_windows_q8 in header, binding and EXPORTS, and the argument
checks of the C launcher (NULL or never-dereferenced handle: nothing is launched)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import subpixel_ref as R
from oracle import cv_ref
from retargetvid_amd import _lib, ops, render, smartVidCrop as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'svc_render_windows_q8'
H, W = 40, 96
PAIRS = [((20, 36), (36, 64)), ((48, 28), (18, 10)), ((20, 36), (20, 36))]      # (bw, bh) -> (ow, oh): up, down, equal
IDS = ['up', 'down', 'equal']


def _frames(n, seed=0, h=H, w=W):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


# ---- the oracle against itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('win,size', PAIRS, ids=IDS)
def test_phase_zero_is_cv_refs_resize_of_the_integer_crop(win, size):
    (bw, bh), (ow, oh) = win, size
    fr = _frames(6)
    xy = np.array([[0, 0], [W - bw, H - bh], [3, 3], [W - bw, 0], [0, H - bh], [7, 2]])
    got = R.windows_rgb(fr, xy * 256, bw, bh, oh, ow)
    for f, (x, y) in enumerate(xy):
        assert np.array_equal(got[f], cv_ref.resize_linear_u8(fr[f, y:y + bh, x:x + bw], oh, ow)), f
    if (oh, ow) == (bh, bw):
        assert np.array_equal(got[2], fr[2, 3:3 + bh, 3:3 + bw])       # the identity table: the crop itself


@pytest.mark.parametrize('win,size', PAIRS, ids=IDS)
def test_a_whole_pixel_of_origin_is_a_whole_pixel_of_source(win, size):
    """Phase (xf, yf) at origin (xi + 1, yi + 1) is phase (xf, yf) at (xi, yi) on the frame moved by one pixel: the taps are
    xi + sx' and yi + sy', so this holds for every column and row, the clamped edge ones included."""
    (bw, bh), (ow, oh) = win, size
    fr = _frames(1, seed=1)
    moved = np.zeros_like(fr)
    moved[:, :-1, :-1] = fr[:, 1:, 1:]
    for xf, yf in ((1, 0), (0, 1), (128, 77), (255, 255), (37, 200)):
        for xi, yi in ((0, 0), (5, 2), (W - bw - 2, H - bh - 2)):
            a = R.windows_rgb(fr, [[(xi + 1) * 256 + xf, (yi + 1) * 256 + yf]], bw, bh, oh, ow)
            b = R.windows_rgb(moved, [[xi * 256 + xf, yi * 256 + yf]], bw, bh, oh, ow)
            assert np.array_equal(a, b), (xf, yf, xi, yi)


def test_a_ramp_moves_monotonically_with_the_phase_and_within_the_rounding_bound():
    """A frame that is x across 256 columns (slope 1, constant in y), a 40-wide window up-scaled to 100 columns.  At phase xf the
    position of an interior column is pos = xi + (sx * 2048 + a1 + 8 xf) / 2048 and the horizontal pass is exact: h = 2048 pos.  The
    vertical pass adds two floors of b * (h >> 4) / 65536 with b0 + b1 = 2048, so S lies in (4 pos - 2 - 1/32, 4 pos], and the value
    floor((S + 2) / 4) in (pos - 1 - 1/128, pos + 1/2].  Every step is monotone in h, so the value never falls as xf grows; one
    unit of phase moves pos by 1/256, the value by at most one grey level."""
    bw, bh, ow, oh, xi, yi = 40, 8, 100, 12, 100, 3
    fr = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], (256, 16, 256, 3)).copy()
    org = np.stack([xi * 256 + np.arange(256), np.full(256, yi * 256 + 99)], 1)
    out = R.windows_rgb(fr, org, bw, bh, oh, ow).astype(np.int64)
    assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    v = out[..., 0]                                             # [xf, oy, ox]: the rows differ in how b0 + b1 = 2048 is split, not in h
    assert (np.diff(v, axis=0) >= 0).all() and (np.diff(v, axis=0) <= 1).all()
    xofs, alpha, xmax = cv_ref._linear_coeffs(bw, ow, float(bw) / ow, True)
    inner = [ox for ox in range(ow) if 0 < xofs[ox] < bw - 2 and ox < xmax]
    assert len(inner) > 80
    for ox in inner:
        for xf in (0, 1, 100, 255):
            pos = xi + Fraction(int(xofs[ox]) * 2048 + int(alpha[ox, 1]) + 8 * xf, 2048)
            assert pos - 1 - Fraction(1, 128) < int(v[xf, :, ox].min()) and int(v[xf, :, ox].max()) <= pos + Fraction(1, 2), (ox, xf)
    assert (v[255][:, inner] - v[0][:, inner]).min() >= 0 and (v[255][:, inner] - v[0][:, inner]).max() >= 1             # (the phase does move the picture)


# ---- sc_compute_bb ------------------------------------------------------------------------------------------------------------------
def _vd(dxs, dys, borders=(0, 0, 0, 0), final=(607, 1080)):
    vd = dict(fc=len(dxs), dxs=list(dxs), dys=list(dys), w_orig=1920, h_orig=1080, w_process=250, h_process=140,
              w_final=final[0], h_final=final[1])
    vd.update(zip(('border_t', 'border_b', 'border_l', 'border_r'), borders))
    return vd


DXS = [-30.5, -0.01, 0.0, 39.4, 39.53, 124.999, 125.0, 200.2, 210.77, 250.0, 400.25, 1e9]
DYS = [70.0, -5.0, 0.3, 69.99, 70.01, 139.9, 140.0, 500.0, 12.5, 70.5, 70.25, -1e9]
CX = [-234, 0, 0, 302, 303, 959, 959, 1537, 1618, 1919, 3073, 7679999999]         # the truncated centres the parent writes back
CY = [540, -38, 2, 539, 540, 1079, 1080, 3857, 96, 543, 541, -7714285714]


@pytest.mark.parametrize('borders,final,want', [
    # (x1, y1) of the parent's boxes and its truncated centres, copied from a run of the parent commit's sc_compute_bb
    ((0, 0, 0, 0), (607, 1080), dict(fbb=(607, 1080), x1=[0, 0, 0, 0, 0, 656, 656, 1234, 1313, 1313, 1313, 1313], y1=[0] * 12)),
    ((0, 0, 100, 60), (607, 1080), dict(fbb=(607, 1080), x1=[100, 100, 100, 100, 100, 656, 656, 1234, 1253, 1253, 1253, 1253], y1=[0] * 12)),
    ((20, 30, 0, 0), (1920, 864), dict(fbb=(1920, 864), x1=[0] * 12, y1=[108, 20, 20, 107, 108, 186, 186, 186, 20, 111, 109, 20])),
])
def test_compute_bb_keeps_the_parents_values_and_adds_the_origins(borders, final, want):
    vd = S.sc_compute_bb(_vd(DXS, DYS, borders, final), S.sc_init_crop_params())
    fw, fh = want['fbb']
    assert (vd['fbb_w'], vd['fbb_h']) == (fw, fh)
    assert vd['dxs'] == CX and vd['dys'] == CY
    assert vd['bbs_np'].dtype == np.int64 and vd['bbs_np'][:, 0].tolist() == want['x1'] and vd['bbs_np'][:, 1].tolist() == want['y1']
    assert np.array_equal(vd['bbs_np'][:, 2:], vd['bbs_np'][:, :2] + [fw, fh]) and vd['bbs'] == vd['bbs_np'].tolist()
    _check_origins(vd, borders)


def _check_origins(vd, borders):
    q8 = vd['bbs_q8']
    bt, bb, bl, br = borders
    assert q8.dtype == np.int64 and q8.shape == (vd['fc'], 2)
    assert np.array_equal(q8 >> 8, vd['bbs_np'][:, :2])                                       # the invariant, on every frame
    # inside the clamp; a window that does not fit between the borders sits at the upper bound, as the parent's box does (its upper clamp comes last)
    for k, lo, hi in ((0, bl * 256, (vd['w_orig'] - br - vd['fbb_w']) * 256), (1, bt * 256, (vd['h_orig'] - bb - vd['fbb_h']) * 256)):
        assert (q8[:, k] <= hi).all() and ((q8[:, k] >= lo).all() if lo <= hi else (q8[:, k] == hi).all())


@pytest.mark.parametrize('borders', [(0, 0, 0, 0), (20, 30, 0, 0), (0, 0, 100, 60), (8, 4, 12, 16)])
@pytest.mark.parametrize('final', [(607, 1080), (1920, 864), (1920, 1080)])
def test_the_origins_truncate_to_the_boxes_on_random_centres(borders, final):
    rs = np.random.RandomState(3)
    dxs = np.concatenate([rs.uniform(-40, 300, 400), np.arange(0, 250, 0.5), [-1e12, 1e12]])
    dys = np.concatenate([rs.uniform(-30, 180, 400), np.arange(500) * 0.28, [1e12, -1e12]])
    vd = S.sc_compute_bb(_vd(dxs, dys, borders, final), S.sc_init_crop_params())
    _check_origins(vd, borders)
    frac = vd['bbs_q8'] & 255
    assert len(np.unique(frac[:, 0])) > 50 or final[0] == 1920                 # (the fractions are kept where the window can move)
    # an unclamped origin IS the smoothed centre: floor(centre * 256) - half the window
    x = np.floor(np.asarray(dxs) / (250 / 1920) * 256) - int(vd['fbb_w'] / 2.0) * 256
    free = (vd['bbs_q8'][:, 0] > borders[2] * 256) & (vd['bbs_q8'][:, 0] < (1920 - borders[3] - vd['fbb_w']) * 256)
    assert np.array_equal(vd['bbs_q8'][free, 0], x[free].astype(np.int64))


# ---- the Python doors ---------------------------------------------------------------------------------------------------------------
def _video(n=4):
    return dict(frames=np.zeros((n, H, W, 3), np.uint8), fr=25.0, frame_count=n, w=W, h=H, trans_inds=[0, n])


def _rvd(n=4, q8=True):
    vd = dict(fc=n, bbs_np=np.array([[2, 4, 22, 40]] * n, np.int64))
    if q8:
        vd['bbs_q8'] = np.array([[2 * 256 + 7, 4 * 256]] * n, np.int64)
    return vd


def test_render_video_refuses_before_any_device_work(monkeypatch):
    monkeypatch.setattr(S, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    with pytest.raises(ValueError) as e:
        render.render_video(_video(), _rvd(), out_size=(36, 64), subpixel=True, interp='lanczos')
    assert "interp='linear'" in str(e.value)
    with pytest.raises(ValueError) as e:
        render.render_video(_video(), _rvd(q8=False), out_size=(36, 64), subpixel=True)
    assert "VD['bbs_q8']" in str(e.value)
    for bad in (np.zeros((4, 4), np.int64), np.zeros((4, 2), np.float64), np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError) as e:
            render.render_video(_video(), dict(_rvd(), bbs_q8=bad), out_size=(36, 64), subpixel=True)
        assert 'integer origins [fc, 2]' in str(e.value)
    # fc = 0 returns before the device, shaped as ever
    empty = dict(fc=0, bbs_np=np.zeros((0, 4), np.int64), bbs_q8=np.zeros((0, 2), np.int64))
    assert render.render_video(_video(), empty, out_size=(36, 64), subpixel=True).shape == (0, 64, 36, 3)


def test_smart_vid_crop_refuses_lanczos_with_subpixel_before_any_work(monkeypatch):
    monkeypatch.setattr(S, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    with pytest.raises(ValueError) as e:
        S.smart_vid_crop(_video(), final_vid_fn='x', out_size=(36, 64), out_interp='lanczos', out_subpixel=True)
    assert "out_interp='linear'" in str(e.value)


def test_smart_vid_crop_forwards_subpixel_only_when_asked(monkeypatch):
    vd = dict(_rvd(), fr=25.0, fbb_w=20, fbb_h=36)
    monkeypatch.setattr(S, 'ingest_frames', lambda *a, **k: dict(vd))
    monkeypatch.setattr(S, 'after_ingest', lambda VD, CP, engine, verbose=False: (VD, {}))
    monkeypatch.setattr(S, '_video_writer', lambda path, fr, size, **kw: type('W', (), dict(write=lambda s, f: None, release=lambda s: None))())
    seen = []
    monkeypatch.setattr(render, 'render_video', lambda video, VD, **kw: seen.append(kw))
    S.smart_vid_crop(_video(), final_vid_fn='a', engine=object())
    S.smart_vid_crop(_video(), final_vid_fn='b', engine=object(), out_size=(36, 64), out_subpixel=True)
    assert 'subpixel' not in seen[0] and seen[1]['subpixel'] is True and seen[1]['out_size'] == (36, 64)


def test_render_windows_refuses_bad_origins_before_any_device_work():
    eng = ops.Engine.__new__(ops.Engine)                        # no handle, no device
    frames = np.zeros((4, H, W, 3), np.uint8)
    for bad in (np.zeros((4, 2), np.int32), torch.zeros((4, 2), dtype=torch.int64), torch.zeros((4, 2), dtype=torch.float32), None):
        with pytest.raises(TypeError) as e:
            eng.render_windows(frames, bad, (20, 36))
        assert 'origins_q8 must be a CUDA tensor of dtype torch.int32' in str(e.value)
    for bad in (torch.zeros((4, 4), dtype=torch.int32), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((8,), dtype=torch.int32)):
        with pytest.raises(ValueError) as e:
            eng.render_windows(frames, bad, (20, 36))
        assert 'origins_q8 of shape' in str(e.value)
    good = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(ValueError):                             # render_crops's own checks, before the tensors are looked at
        eng.render_windows(frames, good, (20, 36), out_hw=(63, 36), out_fmt='nv12')
    with pytest.raises(ValueError):
        eng.render_windows(frames, good, (20, 36), out_fmt='yuv420p')
    with pytest.raises(ValueError):
        eng.render_windows(frames, good, (20, 36), out_colour=('bt709', 'full'))
    with pytest.raises(TypeError):
        eng.render_windows(frames, good, (20, 36), out_layout=dict(pitch=96))
    with pytest.raises(TypeError):                              # a CPU tensor of the right type and shape: the device check
        eng.render_windows(torch.from_numpy(frames), good, (20, 36))


# ---- the C entry --------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    text = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    proto = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % ENTRY, text)
    assert proto, ENTRY + ' is not declared'
    params = [' '.join(p.split()) for p in proto.group(1).split(',')]
    assert params == ['SvcHandle *h', 'const uint8_t *frames', 'const SvcFrameLayout *layout', 'const SvcColour *in_colour', 'int n',
                      'int height', 'int width', 'const int32_t *origins_q8', 'int bw', 'int bh', 'uint8_t *out',
                      'const SvcFrameLayout *out_layout', 'const SvcColour *out_colour', 'int oh', 'int ow', 'int flags', 'void *stream']
    assert _lib.EXPORTS.count(ENTRY) == 1 and ENTRY in _lib.LATER_ENTRIES
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = [i32 if p.startswith('int ') else ctypes.POINTER(_lib.SvcFrameLayout) if 'SvcFrameLayout' in p
            else ctypes.POINTER(_lib.SvcColour) if 'SvcColour' in p else vp for p in params]
    fn = getattr(_lib.load(), ENTRY)
    assert fn.argtypes == want and fn.restype == i32
    history = hdr[hdr.index('ABI revision of the loaded library'):hdr.index('#define SVC_ABI_VERSION')]
    assert ENTRY in history[history.index('(12, no bump)'):history.index(' * 13 = ')]      # it came under revision 12, without a bump
    assert int(re.search(r'#define SVC_ABI_VERSION (\d+)', hdr).group(1)) == 13


def _call(olay, n=0, h=None, frames=None, origins=None, out=None, bw=20, bh=36, oh=64, ow=36, flags=0, out_colour=None, in_fmt='rgb24',
          height=H, width=W):
    lib = _lib.load()
    lay = ops.frame_layout(in_fmt, height, width).struct()
    rc = getattr(lib, ENTRY)(h, frames, ctypes.byref(lay), None, n, height, width, origins, bw, bh, out,
                             ctypes.byref(olay) if olay is not None else None,
                             ctypes.byref(out_colour) if out_colour is not None else None, oh, ow, flags, None)
    return rc, lib.svc_last_error().decode()


def test_the_argument_errors_of_the_launcher():
    rgb, nv = ops.frame_layout('rgb24', 64, 36).struct(), ops.frame_layout('nv12', 64, 36).struct()
    assert _call(None) == (-1, ENTRY + ': out_layout: layout is NULL')
    col = _lib.SvcColour(ctypes.sizeof(_lib.SvcColour), 1, 1, 0)
    rc, msg = _call(rgb, out_colour=col)
    assert rc == -1 and ENTRY + ': out_colour is given but that side is rgb24' in msg
    assert _call(nv, out_colour=col) == (-1, ENTRY + ': invalid argument')          # legal: the next check's answer, the NULL handle
    fake = ctypes.c_void_p(16)                                  # never dereferenced: an argument check answers first
    rc, msg = _call(nv, flags=ops.RENDER_BGR, h=fake)
    assert rc == -1 and 'flags must be 0 (SVC_RENDER_BGR has no meaning for an NV12 output)' in msg
    rc, msg = _call(_lib.SvcFrameLayout(40, 1, 4096, 35, 35 * 64, 36), h=fake)
    assert rc == -1 and "out_layout: pitch 35 is below the row's 36 bytes" in msg
    # n > 0 without origins: refused before anything is touched (frames and out are never dereferenced either)
    assert _call(rgb, n=1, h=fake, frames=fake, out=fake, origins=None) == (-1, ENTRY + ': invalid argument')
    assert _call(rgb, n=0, h=fake)[0] == 0                      # n = 0: a successful no-op, null buffers allowed
    rc, msg = _call(rgb, h=fake, bw=W + 1)
    assert rc == -1 and msg == ENTRY + ': invalid argument'


def test_the_lds_rule_counts_one_more_staged_column():
    """bw = 10901 to 16 output columns: the integer entry needs 2 * 32736 + 64 = 65536 bytes and runs, the sub-pixel entry stages one
    column more -- span = 3 * 10902 + 32 rounded up to 16 = 32752 -- and refuses with the byte count."""
    fake = ctypes.c_void_p(16)
    olay = ops.frame_layout('rgb24', 8, 16).struct()
    rc, msg = _call(olay, h=fake, bw=10901, bh=8, oh=8, ow=16, height=8, width=10902)
    assert rc == -1 and msg == ENTRY + ': window 10901x8 -> 16x8 needs 65568 bytes of LDS per output row (> 64 KiB)'
    lib = _lib.load()
    lay = ops.frame_layout('rgb24', 8, 10902).struct()
    assert lib.svc_render_crops_to_layout(fake, None, ctypes.byref(lay), None, 0, 8, 10902, None, 10901, 8, None, ctypes.byref(olay), None,
                                          8, 16, 0, 0, None) == 0
    assert _call(olay, h=fake, bw=10900, bh=8, oh=8, ow=16, height=8, width=10902)[0] == 0
