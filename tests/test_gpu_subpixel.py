"""-m gpu: sub-pixel crop windows (svc_render_windows_q8, Engine.render_windows, render_video(subpixel=True)) against the NumPy
statement tests/subpixel_ref.py, bit for bit.  Frames are 40 x 96 (NV12-legal); the RGB frames are the NV12 frames converted by
nv12_ref, so one expectation serves both sources.  Every output lies in a poisoned and guarded buffer (tests/poison.py); the tests
that say which bytes are written run under both fills and compare the WHOLE buffer.  Shapes: the three size pairs of the issue (up,
down, equal), and for the staging paths window widths below, at and above one and two 16-pixel groups."""
import functools

import numpy as np
import pytest
import torch

import nv12_ref
import poison
import subpixel_ref as R
from poison import poisoned_outputs  # noqa: F401  (the fixture of the tests that run under one fill)
from retargetvid_amd import ops, render, smartVidCrop as S, synth

pytestmark = pytest.mark.gpu

H, W = 40, 96
DEV = 'cuda'
PAIRS = [((20, 36), (36, 64)), ((48, 28), (18, 10)), ((20, 36), (20, 36))]      # (bw, bh) -> (ow, oh): up, down, equal
IDS = ['up', 'down', 'equal']
SINKS = (('rgb', dict()), ('bgr', dict(bgr=True)), ('nv12', dict(out_fmt='nv12')))
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(params=poison.FILLS, ids=['a5', '5a'])
def guard(request, monkeypatch):
    """One Poison per case: the test's own buffers come from it, and so do the outputs the wrappers allocate."""
    p = poison.Poison(request.param)
    monkeypatch.setattr(ops, 'torch', p)
    yield p
    p.check()


@functools.lru_cache(maxsize=None)
def _pictures(n, seed=21):
    """n random NV12 frames and the RGB frames they convert to, on the host (made once, never changed)."""
    nv = np.random.RandomState(seed).randint(0, 256, (n, H * 3 // 2, W)).astype(np.uint8)
    rgb = nv12_ref.nv12_to_rgb(nv, H, W)
    nv.setflags(write=False)
    rgb.setflags(write=False)
    return dict(nv12=nv, rgb24=rgb)


@functools.lru_cache(maxsize=None)
def _on_device(n, fmt):
    return torch.from_numpy(_pictures(n)[fmt].copy()).to(DEV)


def _org(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1, 2)).to(DEV)


def _expect(crops, sink):
    return R.deliver(crops, 'nv12' if sink == 'nv12' else 'rgb24', bgr=sink == 'bgr')


def _run_all(engine, p, n, origins, win, size):
    """Every source x sink on the first n pictures at `origins`; each result against the oracle's, computed once."""
    (bw, bh), (ow, oh) = win, size
    crops = R.windows_rgb(_pictures(n)['rgb24'], origins, bw, bh, oh, ow)
    for fmt in ops.PIX_FMTS:
        for sink, kw in SINKS:
            got = engine.render_windows(_on_device(n, fmt), _org(origins), (bw, bh), out_hw=(oh, ow), pix_fmt=fmt, **kw)
            p.check()
            assert np.array_equal(got.cpu().numpy(), _expect(crops, sink)), (fmt, sink)
    return crops


# ---- the anchor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('win,size', PAIRS, ids=IDS)
def test_whole_pixel_origins_are_render_crops_byte_for_byte(engine, poisoned_outputs, win, size):
    """Origins that are multiples of 256 -- interior, odd, and flush with each of the four frame edges and corners."""
    (bw, bh), (ow, oh) = win, size
    xy = np.array([[0, 0], [W - bw, H - bh], [W - bw, 0], [0, H - bh], [3, 1], [7, 2], [W - bw - 1, H - bh - 1], [W - bw, 3]])
    n = len(xy)
    boxes = torch.from_numpy(np.concatenate([xy, xy + [bw, bh]], 1).astype(np.int32)).to(DEV)
    for fmt in ops.PIX_FMTS:
        for sink, kw in SINKS:
            want = engine.render_crops(_on_device(n, fmt), boxes, out_hw=(oh, ow), pix_fmt=fmt, **kw)
            got = engine.render_windows(_on_device(n, fmt), _org(xy * 256), (bw, bh), out_hw=(oh, ow), pix_fmt=fmt, **kw)
            poisoned_outputs.check()
            assert torch.equal(got, want), (fmt, sink)
    _run_all(engine, poisoned_outputs, n, xy * 256, win, size)                     # and both are the oracle's


# ---- every phase --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('win,size', PAIRS, ids=IDS)
def test_every_phase_against_the_oracle(engine, poisoned_outputs, win, size):
    """256 frames with xf = 0..255 at a fixed interior origin, 256 with yf = 0..255, then 64 random (X, Y) over the whole clamp
    range -- one call of 576 frames per source and sink."""
    (bw, bh), _ = win, size
    xi, yi = 7, 2
    assert xi < W - bw and yi < H - bh
    k = np.arange(256)
    rs = np.random.RandomState(5)
    rnd = np.stack([rs.randint(0, (W - bw) * 256 + 1, 64), rs.randint(0, (H - bh) * 256 + 1, 64)], 1)
    origins = np.concatenate([np.stack([xi * 256 + k, np.full(256, yi * 256)], 1), np.stack([np.full(256, xi * 256), yi * 256 + k], 1), rnd])
    _run_all(engine, poisoned_outputs, len(origins), origins, win, size)


# ---- clamping -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('win,size', PAIRS, ids=IDS)
def test_bad_origins_are_clamped_into_the_frame(engine, poisoned_outputs, win, size):
    (bw, bh), (ow, oh) = win, size
    mx, my = (W - bw) * 256, (H - bh) * 256
    bad = np.array([[-1, -1], [-256, 77], [300, -100000], [mx + 1, 5], [mx + 256, my + 256], [9, my + 1], [1, 1], [mx - 1, my - 1],
                    [mx, my], [INT32_MIN, INT32_MIN], [INT32_MAX, INT32_MAX], [INT32_MIN, INT32_MAX], [INT32_MAX, 0]], np.int64)
    clamped = np.stack([np.clip(bad[:, 0], 0, mx), np.clip(bad[:, 1], 0, my)], 1)
    crops = _run_all(engine, poisoned_outputs, len(bad), bad, win, size)
    assert np.array_equal(crops, R.windows_rgb(_pictures(len(bad))['rgb24'], clamped, bw, bh, oh, ow))


# ---- staging paths, layouts and the bytes that are written ---------------------------------------------------------------------------
def _up(v, a):
    return (v + a - 1) // a * a


def _scatter(buf, packed, L, first=0):
    """The rows of packed frames (rgb24 [n, h, w, 3] | nv12 [n, h * 3 / 2, w]) at their places in `buf` (1-D, frame 0 at `first`)."""
    for f in range(packed.shape[0]):
        base = first + f * L.frame_stride
        if L.pix_fmt == 'rgb24':
            rows = packed[f].reshape(L.h, 3 * L.w)
            for y in range(L.h):
                buf[base + y * L.pitch:base + y * L.pitch + 3 * L.w] = rows[y]
        else:
            for y in range(L.h):
                buf[base + y * L.pitch:base + y * L.pitch + L.w] = packed[f, y]
            for j in range(L.h // 2):
                o = base + L.chroma_offset + j * L.chroma_pitch
                buf[o:o + L.w] = packed[f, L.h + j]
    return buf


def _in_layouts(fmt):
    """None (packed), a layout with an odd pitch, and one whose values keep the 16-byte paths."""
    if fmt == 'rgb24':
        return (None, ops.frame_layout(fmt, H, W, dict(pitch=3 * W + 5), (3 * W + 5) * H + 3), ops.frame_layout(fmt, H, W, dict(pitch=3 * W + 16)))
    return (None, ops.frame_layout(fmt, H, W, dict(pitch=W + 3, chroma_offset=(W + 3) * (H + 1) + 1, chroma_pitch=W + 1)),
            ops.frame_layout(fmt, H, W, dict(pitch=W + 16, chroma_offset=(W + 16) * (H + 8)), (W + 16) * (H + 8) * 3 // 2 + 32))


def _frames_at(fmt, L, n, offset, pad=0x3C):
    """The first n pictures in layout L (None: packed) inside one buffer at byte `offset` of a 16-aligned start -> the tensor the
    entry takes.  Bytes outside the pictures hold `pad`."""
    pics = _pictures(n)[fmt]
    if L is None:
        L = ops.frame_layout(fmt, H, W)
        size = n * L.frame_stride
    else:
        size = (n - 1) * L.frame_stride + L.extent
    host = _scatter(np.full(offset + size, pad, np.uint8), pics, L, first=offset)
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    body = dev[offset:]
    if fmt == 'rgb24' and L.pitch == 3 * W and L.frame_stride == 3 * W * H:
        return body.view(n, H, W, 3), None
    if fmt == 'nv12' and L.pitch == W and L.chroma_pitch == W and L.frame_stride == W * H * 3 // 2:
        return body.view(n, H * 3 // 2, W), None
    return body.as_strided((n, L.extent), (L.frame_stride, 1)), L


@pytest.mark.parametrize('bw', [16, 17, 31, 47])
def test_staging_paths_and_layouts(engine, guard, bw):
    """bw below, at and above whole 16-pixel groups, so that the extra column is the last of a group, the first of a new one, or
    in the middle; frames 16-aligned and one byte off (the byte paths); packed and pitched frames (an odd pitch, and values that
    keep the 16-byte loads); a packed output and a pitched one, whose every byte outside the pictures must keep the fill."""
    bh, oh, ow = 9, 12, 26
    mx, my = (W - bw) * 256, (H - bh) * 256
    origins = np.array([[mx, my], [mx - 1, my - 1], [0, 0], [255, 255], [5 * 256 + 128, 3 * 256 + 7], [16 * 256 + 1, 1 * 256 + 200]], np.int64)
    n = len(origins)
    crops = R.windows_rgb(_pictures(n)['rgb24'], origins, bw, bh, oh, ow)
    for fmt in ops.PIX_FMTS:
        for L_in in _in_layouts(fmt):
            for offset in (0, 1):
                frames, lay = _frames_at(fmt, L_in, n, offset)
                assert frames.data_ptr() % 16 == offset
                for sink, kw in SINKS:
                    out_fmt = kw.get('out_fmt', 'rgb24')
                    want = _expect(crops, sink)
                    got = engine.render_windows(frames, _org(origins), (bw, bh), out_hw=(oh, ow), pix_fmt=fmt, layout=lay, **kw)
                    guard.check()
                    assert np.array_equal(got.cpu().numpy(), want), (fmt, L_in, offset, sink)
                    row = ow if out_fmt == 'nv12' else 3 * ow
                    for odd in (True, False):                   # a pitched output at two phases: the whole buffer
                        pitch = row + 1 if odd else _up(row + 1, 16)
                        d = dict(pitch=pitch)
                        if out_fmt == 'nv12':
                            d.update(chroma_offset=pitch * oh + 1, chroma_pitch=ow + 3) if odd else d.update(chroma_offset=pitch * (oh + 2))
                        extent = ops.frame_layout(out_fmt, oh, ow, d).extent
                        L = ops.frame_layout(out_fmt, oh, ow, d, extent + 3 if odd else _up(extent, 16) + 16)
                        size = (n - 1) * L.frame_stride + L.extent
                        phase = 9 if odd else 0
                        buf = guard.empty((size,), dtype=torch.uint8, device=DEV, phase=phase)
                        view = buf.as_strided((n, L.extent), (L.frame_stride, 1))
                        assert engine.render_windows(frames, _org(origins), (bw, bh), out_hw=(oh, ow), out=view, pix_fmt=fmt, layout=lay,
                                                     out_layout=L, **kw) is view
                        guard.check()
                        exp = _scatter(np.full(size, guard.fill, np.uint8), want, L)
                        assert np.array_equal(buf.cpu().numpy(), exp), (fmt, L_in, offset, sink, odd)


# ---- the read range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('win,size', PAIRS[:2], ids=IDS[:2])
def test_no_byte_outside_the_pictures_reaches_a_result(engine, poisoned_outputs, win, size):
    """The frames are a view whose last frame ends exactly where the surrounding buffer's tail begins, and whose rows are followed
    by padding.  Windows flush right and bottom with zero phase (the column xi + bw and the row yi + bh do not exist), and one
    unit short of flush with phase 255 (they are the frame's last).  Padding and tail hold 0x00, then 0xFF: the outputs are the
    oracle's both times.  Nothing is provoked: every address the kernels form lies inside the buffer either way."""
    (bw, bh), (ow, oh) = win, size
    mx, my = (W - bw) * 256, (H - bh) * 256
    origins = np.array([[mx, my], [mx - 1, my - 1], [mx, my - 1], [mx - 1, my], [mx, 0], [0, my]], np.int64)
    n = len(origins)
    crops = R.windows_rgb(_pictures(n)['rgb24'], origins, bw, bh, oh, ow)
    for fmt in ops.PIX_FMTS:
        for L_in in _in_layouts(fmt)[1:]:
            size = (n - 1) * L_in.frame_stride + L_in.extent
            for offset in (0, 1):
                results = []
                for pad in (0x00, 0xFF):
                    host = _scatter(np.full(offset + size + 256, pad, np.uint8), _pictures(n)[fmt], L_in, first=offset)
                    dev = torch.from_numpy(host).to(DEV)
                    frames = dev[offset:offset + size].as_strided((n, L_in.extent), (L_in.frame_stride, 1))
                    for sink, kw in SINKS:
                        got = engine.render_windows(frames, _org(origins), (bw, bh), out_hw=(oh, ow), pix_fmt=fmt, layout=L_in, **kw)
                        poisoned_outputs.check()
                        results.append(got.cpu().numpy())
                        assert np.array_equal(results[-1], _expect(crops, sink)), (fmt, L_in, offset, pad, sink)
                for a, b in zip(results[:3], results[3:]):
                    assert np.array_equal(a, b)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_render_video_follows_the_smoothed_trajectory(engine):
    """One synthetic video through smart_vid_crop(save_vid=False): render_video(subpixel=True) is the oracle applied to
    VD['bbs_q8']; subpixel=False gives the bytes it gives today (the oracle at the whole-pixel origins, i.e. cv_ref's resize of the
    integer crops); the writer mode forwards out_subpixel."""
    video = dict(frames=synth.blob_frames(30, H, W, seed=3), fr=25.0, frame_count=30, w=W, h=H, trans_inds=[0, 30])
    CP = dict(S.sc_init_crop_params(), out_ratio='1:2')
    VD, _ = S.smart_vid_crop(video, CP, save_vid=False, engine=engine)
    fc, bw, bh = int(VD['fc']), int(VD['fbb_w']), int(VD['fbb_h'])
    q8 = np.asarray(VD['bbs_q8'])
    assert fc == 30 and (bw, bh) == (20, 40) and np.array_equal(q8 >> 8, VD['bbs_np'][:, :2])
    assert ((q8[:, 0] & 255) != 0).any()                        # (the smoothed centres do carry a fraction)
    for kw in (dict(out_size=(36, 64)), dict(out_size=(36, 64), out_fmt='nv12'), dict(out_size=(36, 64), bgr=True), dict()):
        ow, oh = kw.get('out_size', (bw, bh))
        out_fmt = kw.get('out_fmt', 'rgb24')
        sub = render.render_video(video, VD, engine=engine, chunk=16, subpixel=True, **kw)
        want = R.deliver(R.windows_rgb(video['frames'], q8, bw, bh, oh, ow), out_fmt, kw.get('bgr', False))
        assert np.array_equal(sub, want), kw
        whole = render.render_video(video, VD, engine=engine, chunk=16, **kw)
        today = R.deliver(R.windows_rgb(video['frames'], (q8 >> 8) << 8, bw, bh, oh, ow), out_fmt, kw.get('bgr', False))
        assert np.array_equal(whole, today) and np.array_equal(whole, render.render_video(video, VD, engine=engine, chunk=16, subpixel=False, **kw))
        assert not np.array_equal(sub, whole)
    lay = dict(pitch=128)                                       # with an out_layout: the same picture bytes, 0 elsewhere
    L = ops.frame_layout('rgb24', 64, 36, lay)
    got = render.render_video(video, VD, engine=engine, out_size=(36, 64), out_layout=lay, subpixel=True)
    want = R.windows_rgb(video['frames'], q8, bw, bh, 64, 36)
    assert np.array_equal(got.ravel(), _scatter(np.zeros(fc * L.frame_stride, np.uint8), want, L))
    # the writer mode
    written = []

    class Writer:
        def __init__(self, path, fr, size, **kw):
            self.size = size

        def write(self, f):
            written.append(np.array(f))

        def release(self):
            pass
    old = S._video_writer
    S.set_video_writer(Writer)
    try:
        S.smart_vid_crop(video, CP, final_vid_fn='a', engine=engine, out_size=(36, 64), out_subpixel=True)
    finally:
        S.set_video_writer(old)
    assert np.array_equal(np.stack(written), want)
