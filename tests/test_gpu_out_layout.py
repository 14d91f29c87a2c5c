"""-m gpu: rendering into an output layout (svc_render_crops_to_layout, Engine.render_crops(out_layout=), render_video(out_layout=)).
The contract: the picture bytes of a pitched output are bit for bit the bytes of the packed output, and every other byte of the
caller's buffer is left untouched.  Every output lies in a poisoned and guarded buffer (tests/poison.py) of exactly (n - 1) *
frame_stride + extent bytes; the expected buffer is built on the host -- the fill everywhere, the rows of the existing packed call's
result (whose own tests pin it to the oracles) scattered to their places -- and the WHOLE buffer must equal it under both fills: a byte
that equals the fill under both fills was not written, a picture byte that equals its reference under both was.  Shapes: the
smallest at which each path can go wrong (a row's last partial group, one and several groups per row, rows on 8 but not 16 bytes,
odd pitches, a chroma plane at an odd offset, several workgroups, a Lanczos band boundary inside the picture)."""
import ctypes

import numpy as np
import pytest
import torch

import nv12_ref
import poison
from retargetvid_amd import _lib, ops, render, smartVidCrop as S

pytestmark = pytest.mark.gpu

N, H, W = 3, 38, 70
DEV = 'cuda'


@pytest.fixture(params=poison.FILLS, ids=['a5', '5a'])
def guard(request, monkeypatch):
    """One Poison per case: the test's own output buffers come from it, and so do the outputs the wrappers allocate."""
    p = poison.Poison(request.param)
    monkeypatch.setattr(ops, 'torch', p)
    yield p
    p.check()


def _up(v, a):
    return (v + a - 1) // a * a


_SRC = {}


def _sources():
    """Random NV12 frames and the RGB frames they convert to, on the device (made once)."""
    if not _SRC:
        nv = np.random.RandomState(11).randint(0, 256, (N, H * 3 // 2, W)).astype(np.uint8)
        _SRC['nv12'] = torch.from_numpy(nv).to(DEV)
        _SRC['rgb24'] = torch.from_numpy(nv12_ref.nv12_to_rgb(nv, H, W)).to(DEV)
    return _SRC


def _boxes(bw, bh):
    """Windows at odd origins; the last one touches the frame's corner."""
    return np.array([[1, 1, 1 + bw, 1 + bh], [3, 5, 3 + bw, 5 + bh], [W - bw, H - bh, W, H]], np.int32)


_PACKED = {}


def _packed(engine, fmt, bw, bh, out_hw, **kw):
    """The existing packed call's result on the host (computed once per case, never changed)."""
    key = (fmt, bw, bh, out_hw, tuple(sorted(kw.items())))
    if key not in _PACKED:
        boxes = torch.from_numpy(_boxes(bw, bh)).to(DEV)
        _PACKED[key] = engine.render_crops(_sources()[fmt], boxes, out_hw=out_hw, pix_fmt=fmt, **kw).cpu().numpy()
        _PACKED[key].setflags(write=False)
    return _PACKED[key]


def _scatter(buf, packed, L, first=0):
    """The rows of the packed frames at their places in `buf` (1-D, frame 0 at `first`)."""
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


def _expected(fill, packed, L):
    return _scatter(np.full((packed.shape[0] - 1) * L.frame_stride + L.extent, fill, np.uint8), packed, L)


def _render_into(engine, guard, fmt, bw, bh, L, phase, out_hw=None, **kw):
    """One call into a poisoned buffer of exactly (N - 1) * frame_stride + extent bytes at `phase` -> does the whole buffer equal
    the expected one (guards checked)."""
    packed = _packed(engine, fmt, bw, bh, out_hw, out_fmt=L.pix_fmt, **kw)
    size = (N - 1) * L.frame_stride + L.extent
    buf = guard.empty((size,), dtype=torch.uint8, device=DEV, phase=phase)
    assert buf.data_ptr() % 16 == phase
    out = buf.as_strided((N, L.extent), (L.frame_stride, 1))
    boxes = torch.from_numpy(_boxes(bw, bh)).to(DEV)
    got = engine.render_crops(_sources()[fmt], boxes, out_hw=out_hw, out=out, pix_fmt=fmt, out_fmt=L.pix_fmt, out_layout=L, **kw)
    assert got is out
    guard.check()
    return np.array_equal(buf.cpu().numpy(), _expected(guard.fill, packed, L))


# ---- the copy to RGB ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [1, 15, 16, 17, 33, 48])
def test_rgb_copy(engine, guard, bw):
    """Output = window.  bw below, at and above one 16-pixel group, with and without a partial last group; the packed pitch, an odd
    one and 16- / 64-aligned ones; frames adjacent, one byte apart and 16-aligned; out at phases 0, 1, 8, 15: the row vector
    kernel where every row starts on 16 bytes, the byte kernel elsewhere, the packed kernels for the packed values."""
    bh = 3
    for pitch in sorted({3 * bw, 3 * bw + 1, _up(3 * bw, 16), _up(3 * bw, 64)}):
        extent = pitch * (bh - 1) + 3 * bw
        for stride in sorted({extent, extent + 1, _up(extent, 16)}):
            L = ops.frame_layout('rgb24', bh, bw, dict(pitch=pitch), stride)
            for phase in (0, 1, 8, 15):
                for fmt in ops.PIX_FMTS:
                    for bgr in (False, True):
                        assert _render_into(engine, guard, fmt, bw, bh, L, phase, bgr=bgr), (pitch, stride, phase, fmt, bgr)


# ---- the copy to NV12 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bh', [2, 6])
@pytest.mark.parametrize('bw', [2, 14, 16, 24, 40])
def test_nv12_copy(engine, guard, bw, bh):
    """The vector kernel stores 8- and 16-byte words: it runs where out, frame_stride, pitch, chroma_offset and chroma_pitch are all
    multiples of 8 (bw % 8 == 0, bw >= 16) -- rows on 8 but not 16 bytes included -- and the byte kernel everywhere else.  Every
    pair of the four pitches and the four chroma pitches runs."""
    choice = (bw, bw + 1, (bw // 8 + 1) * 8, (bw // 16 + 1) * 16)        # packed, odd, the next multiple of 8, of 16
    for ip, ic in ((i, j) for i in range(4) for j in range(4)):
        pitch, cpitch = choice[ip], choice[ic]
        for coff in (pitch * bh, pitch * (bh + 2), pitch * (bh + 2) + 1):
            extent = coff + cpitch * (bh // 2 - 1) + bw
            for stride in ((extent, _up(extent + 1, 8)) if ip == ic else (_up(extent + 1, 8),)):
                L = ops.frame_layout('nv12', bh, bw, dict(pitch=pitch, chroma_offset=coff, chroma_pitch=cpitch), stride)
                for phase in (0, 4, 8):
                    for fmt in ops.PIX_FMTS:
                        assert _render_into(engine, guard, fmt, bw, bh, L, phase), (pitch, cpitch, coff, stride, phase, fmt)


# ---- INTER_LINEAR and Lanczos ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_hw', [(2, 2), (6, 10), (18, 34), (40, 50)], ids=lambda s: '%dx%d' % s[::-1])
@pytest.mark.parametrize('interp', ops.INTERPS)
def test_resampled(engine, guard, interp, out_hw):
    """One 24 x 16 window down and up, both filters, both sinks (and BGR), both sources; an odd and a 16-aligned pitch, a chroma
    plane at an odd offset and behind a coded height; out at phases 0 and 9.  40 output rows are two Lanczos bands (B <= 32)."""
    bw, bh = 24, 16
    oh, ow = out_hw
    for out_fmt in ops.OUT_FMTS:
        row = ow if out_fmt == 'nv12' else 3 * ow
        for odd in (True, False):
            pitch = row + 1 if odd else _up(row + 1, 16)
            lay = dict(pitch=pitch)
            if out_fmt == 'nv12':
                lay.update(chroma_offset=pitch * oh + 1, chroma_pitch=ow + 3) if odd else lay.update(chroma_offset=pitch * (oh + 2))
            extent = ops.frame_layout(out_fmt, oh, ow, lay).extent
            L = ops.frame_layout(out_fmt, oh, ow, lay, extent + 3 if odd else _up(extent, 16) + 16)
            assert L.pitch % 2 == (1 if odd else 0)
            for phase in (0, 9):
                for fmt in ops.PIX_FMTS:
                    for kw in ((dict(), dict(bgr=True)) if out_fmt == 'rgb24' else (dict(),)):
                        assert _render_into(engine, guard, fmt, bw, bh, L, phase, out_hw=out_hw, interp=interp, **kw), (out_fmt, odd, phase, fmt, kw)


# ---- a layout with the packed values --------------------------------------------------------------------------------------------
def _cptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('out_fmt', ops.OUT_FMTS)
def test_the_packed_layout_gives_the_packed_entrys_bytes(engine, guard, out_fmt):
    """The copy, INTER_LINEAR and Lanczos with a layout whose values are the packed ones: the bytes of Engine.render_crops without
    one, and of svc_render_crops_colour called beside the new entry on the same inputs (C ABI, non-default colours)."""
    lib = engine.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (bw, bh), out_hw, interp in (((24, 16), None, 'linear'), ((17, 5), None, 'linear'), ((24, 16), (18, 34), 'linear'),
                                     ((24, 16), (40, 50), 'lanczos')):
        if out_fmt == 'nv12' and (bw % 2 or bh % 2):
            bw, bh = bw + 1, bh + 1
        oh, ow = out_hw or (bh, bw)
        L = ops.frame_layout(out_fmt, oh, ow)
        assert L.frame_stride == L.extent == int(np.prod(ops.frame_shape(out_fmt, oh, ow)))
        for fmt in ops.PIX_FMTS:
            for phase in (0, 5):
                assert _render_into(engine, guard, fmt, bw, bh, L, phase, out_hw=out_hw, interp=interp), (bw, bh, out_hw, interp, fmt, phase)
            # the two C entries side by side
            src = _sources()[fmt]
            lay = ops.frame_layout(fmt, H, W).struct()
            olay = L.struct()
            cin = ops._colour_struct(('bt709', 'full')) if fmt == 'nv12' else None
            cout = ops._colour_struct(('bt709', 'limited')) if out_fmt == 'nv12' else None
            boxes = torch.from_numpy(_boxes(bw, bh)).to(DEV)
            a = guard.empty((N * L.frame_stride,), dtype=torch.uint8, device=DEV)
            b = guard.empty((N * L.frame_stride,), dtype=torch.uint8, device=DEV)
            _lib.check(lib.svc_render_crops_colour(engine._h, _cptr(src), ctypes.byref(lay), cin, N, H, W, _cptr(boxes), bw, bh, _cptr(a),
                                                   ops.OUT_FMTS.index(out_fmt), cout, oh, ow, ops.INTERPS.index(interp), 0, stream))
            _lib.check(lib.svc_render_crops_to_layout(engine._h, _cptr(src), ctypes.byref(lay), cin, N, H, W, _cptr(boxes), bw, bh, _cptr(b),
                                                      ctypes.byref(olay), cout, oh, ow, ops.INTERPS.index(interp), 0, stream))
            guard.check()
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a, b) and (a != guard.fill).any(), (bw, bh, out_hw, interp, fmt)


# ---- out= as a view into a surface pool -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_fmt', ops.OUT_FMTS)
def test_out_is_a_strided_view_into_a_larger_pool(engine, guard, out_fmt):
    """Seven surfaces in one poisoned allocation, the three frames rendered into surfaces 1, 3 and 5 through pool[1:6:2]: the
    surfaces between and around them, and every padding byte of the three, keep the fill."""
    bw, bh, out_hw = 24, 16, (18, 34)
    oh, ow = out_hw
    lay = dict(pitch=64, chroma_offset=64 * 24) if out_fmt == 'nv12' else dict(pitch=112)
    surface = 64 * 36 if out_fmt == 'nv12' else 112 * 20
    one = ops.frame_layout(out_fmt, oh, ow, lay, surface)
    L = one.every(2)
    for interp in ops.INTERPS:
        packed = _packed(engine, 'nv12', bw, bh, out_hw, out_fmt=out_fmt, interp=interp)
        pool = guard.empty((7 * surface,), dtype=torch.uint8, device=DEV)
        view = pool.view(7, surface)[1:6:2]
        assert tuple(view.stride()) == (2 * surface, 1) and view.shape[0] == N
        boxes = torch.from_numpy(_boxes(bw, bh)).to(DEV)
        got = engine.render_crops(_sources()['nv12'], boxes, out_hw=out_hw, out=view, pix_fmt='nv12', out_fmt=out_fmt, out_layout=L,
                                  interp=interp)
        assert got is view
        guard.check()
        want = _scatter(np.full(7 * surface, guard.fill, np.uint8), packed, L, first=surface)
        assert np.array_equal(pool.cpu().numpy(), want), interp
    # a view that does not hold the layout is refused by the door, as for frames
    with pytest.raises(ValueError) as e:
        engine.render_crops(_sources()['nv12'], boxes, out_hw=out_hw, out=pool.view(7, surface)[1:4], pix_fmt='nv12', out_fmt=out_fmt,
                            out_layout=L)
    assert 'out of shape' in str(e.value) and 'bytes apart' in str(e.value)
    with pytest.raises(ValueError) as e:                        # a view with another frame count than the frames
        engine.render_crops(_sources()['nv12'], boxes, out_hw=out_hw, out=pool.view(7, surface)[1:4:2], pix_fmt='nv12', out_fmt=out_fmt,
                            out_layout=L)
    assert 'out holds 2 frames, frames holds 3' in str(e.value)
    # without out= the door allocates [n, frame_stride]
    got = engine.render_crops(_sources()['nv12'], boxes, out_hw=out_hw, pix_fmt='nv12', out_fmt=out_fmt, out_layout=one)
    assert tuple(got.shape) == (N, surface) and got.dtype == torch.uint8
    want = _scatter(np.full(N * surface, guard.fill, np.uint8), _packed(engine, 'nv12', bw, bh, out_hw, out_fmt=out_fmt, interp='linear'), one)
    assert np.array_equal(got.cpu().numpy().ravel(), want)


# ---- render_video end to end ----------------------------------------------------------------------------------------------------
def _video(n=40, h=36, w=64):
    rgb = np.random.RandomState(5).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    x = (np.arange(n) * 3) % (w - 24)
    y = np.arange(n) % (h - 20)
    vd = dict(fc=n, bbs_np=np.stack([x, y, x + 24, y + 20], 1).astype(np.int64))
    return dict(frames=rgb, fr=25.0, frame_count=n, w=w, h=h, trans_inds=[0, n]), vd


@pytest.mark.parametrize('kw', [dict(), dict(out_size=(30, 44)), dict(out_size=(30, 44), interp='lanczos')],
                         ids=['copy', 'linear', 'lanczos'])
def test_render_video_end_to_end(engine, kw):
    """A host container of 40 frames of 36 x 64, windows of 24 x 20 that move, out_layout=dict(pitch=...): the picture bytes are the
    packed render_video's, every other byte is 0, the chunks arrive in order and are [m, frame_stride]; both output formats and a
    non-default out_colour."""
    video, vd = _video()
    ow, oh = kw.get('out_size', (24, 20))
    for out_fmt, lay, more in (('rgb24', dict(pitch=128), dict()), ('rgb24', dict(pitch=3 * ow + 1), dict(bgr=True)),
                               ('nv12', dict(pitch=64, chroma_offset=64 * 48), dict()),
                               ('nv12', dict(pitch=ow + 1, chroma_pitch=ow + 3), dict(out_colour=('bt709', 'full')))):
        packed = render.render_video(video, vd, engine=engine, chunk=16, out_fmt=out_fmt, **kw, **more)
        L = ops.frame_layout(out_fmt, oh, ow, lay)
        chunks = []
        assert render.render_video(video, vd, engine=engine, chunk=16, out_fmt=out_fmt, out_layout=lay, sink=lambda c: chunks.append(c.copy()),
                                   **kw, **more) is None
        assert [c.shape for c in chunks] == [(16, L.frame_stride), (16, L.frame_stride), (8, L.frame_stride)]
        got = np.concatenate(chunks)
        want = _scatter(np.zeros(40 * L.frame_stride, np.uint8), packed, L).reshape(40, L.frame_stride)
        assert np.array_equal(got, want), (out_fmt, lay)
        whole = render.render_video(video, vd, engine=engine, chunk=16, out_fmt=out_fmt, out_layout=L, **kw, **more)     # the checked object
        assert whole.shape == (40, L.frame_stride) and np.array_equal(whole, want)
    assert (packed != 0).mean() > 0.9                           # (the pictures are not what the padding is)


def test_smart_vid_crop_hands_the_writer_pitched_frames(engine, monkeypatch):
    """The whole path once: the installed writer is opened with layout= and receives frames of frame_stride bytes whose picture
    bytes are those of the run without a layout."""
    from retargetvid_amd import synth
    video = dict(frames=synth.blob_frames(30, 36, 64, seed=3), fr=25.0, frame_count=30, w=64, h=36, trans_inds=[0, 30])
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    runs = []

    class Writer:
        def __init__(self, path, fr, size, **kw):
            self.kw, self.size, self.frames = kw, size, []
            runs.append(self)

        def write(self, f):
            self.frames.append(np.array(f))

        def release(self):
            pass
    monkeypatch.setattr(S, '_video_writer', Writer)
    S.smart_vid_crop(video, CP, final_vid_fn='a', engine=engine, out_size=(20, 30), out_pix_fmt='nv12')
    S.smart_vid_crop(video, CP, final_vid_fn='b', engine=engine, out_size=(20, 30), out_pix_fmt='nv12', out_layout=dict(pitch=32, chroma_offset=32 * 32))
    L = ops.frame_layout('nv12', 30, 20, dict(pitch=32, chroma_offset=32 * 32))
    assert runs[0].kw == dict(pix_fmt='nv12') and runs[1].kw == dict(pix_fmt='nv12', layout=L)
    packed, pitched = np.stack(runs[0].frames), np.stack(runs[1].frames)
    assert packed.shape == (30, 45, 20) and pitched.shape == (30, L.frame_stride)
    assert np.array_equal(pitched.ravel(), _scatter(np.zeros(30 * L.frame_stride, np.uint8), packed, L))


# ---- the documented call --------------------------------------------------------------------------------------------------------
def test_the_integration_snippet_runs_as_written(engine):
    """INTEGRATION.md's svc_render_crops_to_layout block, executed as written on two 1080p decoder surfaces: the picture bytes of the
    encoder surfaces are those of the packed entry, the rest keeps its fill."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'INTEGRATION.md')).read()
    m = re.search(r'```python\n(_L\.svc_render_crops_to_layout\.argtypes.*?)```', text, flags=re.S)
    assert m, 'INTEGRATION.md no longer holds the svc_render_crops_to_layout block'
    n = 2
    surfaces = torch.randint(0, 256, (n, 2048 * 1632), dtype=torch.uint8, device=DEV)
    lay = ops.frame_layout('nv12', 1080, 1920, dict(pitch=2048, chroma_offset=2048 * 1088), 2048 * 1632)
    boxes = torch.tensor([[100, 0, 708, 1080], [1311, 0, 1919, 1080]], dtype=torch.int32, device=DEV)
    enc = torch.full((n, 1280 * 2880), 0xA5, dtype=torch.uint8, device=DEV)
    ns = dict(ctypes=ctypes, _L=engine.lib, vp=ctypes.c_void_p, i32=ctypes.c_int, SvcFrameLayout=_lib.SvcFrameLayout, SvcColour=_lib.SvcColour,
              SVC_FMT_NV12=_lib.FMT_NV12, h=engine._h, surfaces_ptr=_cptr(surfaces), lay=lay.struct(), n=n, boxes_ptr=_cptr(boxes),
              enc_surfaces_ptr=_cptr(enc), stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    exec(compile(m.group(1), 'INTEGRATION.md:svc_render_crops_to_layout', 'exec'), ns)
    assert ns['rc'] == 0, engine.lib.svc_last_error()
    packed = engine.render_crops(surfaces, boxes, out_hw=(1920, 1080), pix_fmt='nv12', out_fmt='nv12', layout=lay).cpu().numpy()
    L = ops.frame_layout('nv12', 1920, 1080, dict(pitch=1280, chroma_offset=1280 * 1920), 1280 * 2880)
    assert ns['olay'].frame_stride == L.frame_stride and ns['olay'].chroma_offset == L.chroma_offset
    assert np.array_equal(enc.cpu().numpy().ravel(), _scatter(np.full(n * L.frame_stride, 0xA5, np.uint8), packed, L))
