"""-m gpu: the renderer's Lanczos filter (svc_render_crops_filter, k_render_lanczos and every door above them: interp='lanczos' of
ops.Engine.render_crops and render.render_video, out_interp='lanczos' of smart_vid_crop).  Every expected RGB crop is
oracle.lanczos_ref.resize_lanczos_u8 -- Pillow's resize(LANCZOS) restated, pinned to Pillow by tests/golden -- of the NumPy slice of
the frame (of nv12_ref.nv12_to_rgb(frame) for NV12 input); BGR is its [..., ::-1], NV12 output is nv12_out_ref.rgb_to_nv12_fixed of
it.  Every comparison is np.array_equal; nothing has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import nv12_out_ref
import nv12_ref
from oracle import lanczos_ref
from retargetvid_amd import _lib, ingest, ops, render, smartVidCrop as S, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

forward = nv12_out_ref.rgb_to_nv12_fixed
N, H, W = 5, 360, 640
# (bw, bh) -> (oh, ow)
SHAPES = (((101, 180), (320, 180)),         # non-integer upscale
          ((270, 360), (160, 120)),         # 2.25x down, wide kernel
          ((301, 77), (50, 333)),           # one axis up and one down
          ((120, 90), (90, 200)),           # vertical pass skipped
          ((120, 90), (45, 120)),           # horizontal pass skipped
          ((640, 360), (36, 64)),           # 10x down, kernel of 61 taps
          ((1, 1), (5, 7)),                 # degenerate windows
          ((3, 2), (2, 2)),
          ((17, 5), (33, 31)))              # oh not a multiple of any band
BIG = ((1080, 1920), (607, 1080), (1920, 1080))          # one 1080p frame: another band size B than the small cases
NV12_SOURCE_SHAPES = (SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[8])
IDS = ['%dx%d-%dx%d' % (bw, bh, ow, oh) for (bw, bh), (oh, ow) in SHAPES]


def _boxes(n, h, w, bw, bh, seed):
    """n windows of bw x bh: the four corners of the frame first (every edge touched), then origins odd in x and y where the frame
    leaves room."""
    rng = np.random.RandomState(seed)
    xs = [0, w - bw, 0, w - bw] + [min(int(v) | 1, w - bw) for v in rng.randint(0, max(w - bw, 1), n)]
    ys = [0, 0, h - bh, h - bh] + [min(int(v) | 1, h - bh) for v in rng.randint(0, max(h - bh, 1), n)]
    return np.array([[x, y, x + bw, y + bh] for x, y in zip(xs[:n], ys[:n])], np.int32)


def _expect(rgb, boxes, oh, ow):
    return np.stack([lanczos_ref.resize_lanczos_u8(np.ascontiguousarray(f[y1:y2, x1:x2]), oh, ow)
                     for f, (x1, y1, x2, y2) in zip(rgb, boxes)])


class _Pictures:
    """The frames of one source format, on the host (as fed, and as RGB) and on the device, and every expectation asked for so
    far: a reference is computed once and shared by the tests that need it."""

    def __init__(self, pix_fmt, n, h, w, seed):
        rng = np.random.RandomState(seed)
        self.pix_fmt, self.n, self.h, self.w = pix_fmt, n, h, w
        if pix_fmt == 'nv12':
            self.fed = rng.randint(0, 256, (n, h * 3 // 2, w)).astype(np.uint8)
            self.rgb = nv12_ref.nv12_to_rgb(self.fed, h, w)
        else:
            self.fed = self.rgb = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        self.dev = torch.from_numpy(self.fed).cuda()
        self._exp = {}

    def boxes(self, bw, bh):
        return _boxes(self.n, self.h, self.w, bw, bh, seed=bw + bh)

    def expect(self, bw, bh, oh, ow):
        key = (bw, bh, oh, ow)
        if key not in self._exp:
            e = _expect(self.rgb, self.boxes(bw, bh), oh, ow)
            e.setflags(write=False)
            self._exp[key] = e
        return self._exp[key]


@pytest.fixture(scope='module')
def pictures():
    return {'rgb24': _Pictures('rgb24', N, H, W, seed=11), 'nv12': _Pictures('nv12', N, H, W, seed=12)}


def _check_all_sinks(engine, pic, bw, bh, oh, ow, frames=None, layout=None):
    """RGB and BGR on every shape, NV12 where the output is even: against the oracle."""
    d = pic.dev if frames is None else frames
    boxes, exp = pic.boxes(bw, bh), pic.expect(bw, bh, oh, ow)
    kw = dict(out_hw=(oh, ow), pix_fmt=pic.pix_fmt, layout=layout, interp='lanczos')
    got = engine.render_crops(d, torch.from_numpy(boxes).cuda(), **kw)
    assert got.shape == exp.shape and np.array_equal(got.cpu().numpy(), exp), 'rgb'
    got = engine.render_crops(d, boxes, bgr=True, **kw)
    assert np.array_equal(got.cpu().numpy(), exp[..., ::-1]), 'bgr'
    if oh % 2 == 0 and ow % 2 == 0:
        got = engine.render_crops(d, boxes, out_fmt='nv12', **kw)
        assert got.shape == (pic.n, oh * 3 // 2, ow) and np.array_equal(got.cpu().numpy(), forward(exp)), 'nv12'


@pytest.mark.parametrize('win,osz', SHAPES, ids=IDS)
def test_every_sink_on_every_shape(engine, pictures, win, osz):
    _check_all_sinks(engine, pictures['rgb24'], *win, *osz)


def test_one_1080p_frame(engine):
    (h, w), (bw, bh), (oh, ow) = BIG
    pic = _Pictures('rgb24', 2, h, w, seed=13)               # windows at x = 0 and at the right edge, x = 1313
    _check_all_sinks(engine, pic, bw, bh, oh, ow)


@pytest.mark.parametrize('win,osz', NV12_SOURCE_SHAPES)
def test_nv12_source(engine, pictures, win, osz):
    """Windows at origins odd in x and in y: the chroma index comes from frame coordinates."""
    pic = pictures['nv12']
    b = pic.boxes(*win)
    assert (b[4, 0] & 1) and (b[4, 1] & 1)
    _check_all_sinks(engine, pic, *win, *osz)


def _pitched(packed, fmt, h, w, pitch, coded_h, chroma_pitch, frame_stride, fill):
    """The packed pictures as surfaces with these strides in a device buffer full of `fill` -> (uint8 [n, frame_stride], layout)."""
    n = packed.shape[0]
    lay = dict(pitch=pitch)
    if fmt == 'nv12':
        lay.update(chroma_offset=pitch * coded_h, chroma_pitch=chroma_pitch)
    L = ops.frame_layout(fmt, h, w, lay, frame_stride)
    buf = np.full((n, L.frame_stride), fill, np.uint8)
    view = np.lib.stride_tricks.as_strided
    if fmt == 'nv12':
        view(buf, (n, h, w), (L.frame_stride, L.pitch, 1))[...] = packed[:, :h]
        view(buf.reshape(-1)[L.chroma_offset:], (n, h // 2, w), (L.frame_stride, L.chroma_pitch, 1))[...] = packed[:, h:]
    else:
        view(buf, (n, h, 3 * w), (L.frame_stride, L.pitch, 1))[...] = packed.reshape(n, h, 3 * w)
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    return dev, L


@pytest.mark.parametrize('pix_fmt', ops.PIX_FMTS)
@pytest.mark.parametrize('kind', ('odd', 'decoder'))
def test_pitched_layouts_equal_the_packed_call(engine, pictures, pix_fmt, kind):
    """An odd pitch and frame_stride (NV12: every U V pair may lie on an odd address, the byte staging path) and a decoder's
    even ones (pitch a multiple of 256, coded height above the picture's: the 16-byte staging path), every padding byte 0xFF.
    The bytes of the packed call, which are the oracle's."""
    pic = pictures[pix_fmt]
    row = W if pix_fmt == 'nv12' else 3 * W
    if kind == 'odd':
        pitch, coded_h, cp = row + 1, H + 1, row + 3
    else:
        pitch, coded_h, cp = (row + 255) // 256 * 256, H + 8, (row + 255) // 256 * 256
    extent = ops.frame_layout(pix_fmt, H, W, dict(pitch=pitch, chroma_offset=pitch * coded_h, chroma_pitch=cp) if pix_fmt == 'nv12'
                              else dict(pitch=pitch)).extent
    stride = extent + (4096 + extent % 2 if kind == 'decoder' else 5 + extent % 2)           # decoder: even; odd: odd
    assert stride % 2 == (kind == 'odd') and pitch % 2 == (kind == 'odd')
    dev, L = _pitched(pic.fed, pix_fmt, H, W, pitch, coded_h, cp, stride, 0xFF)
    for (bw, bh), (oh, ow) in (SHAPES[0], SHAPES[1]):
        boxes = pic.boxes(bw, bh)
        for out_fmt, bgr in (('rgb24', False), ('rgb24', True), ('nv12', False)):
            kw = dict(out_hw=(oh, ow), bgr=bgr, pix_fmt=pix_fmt, out_fmt=out_fmt, interp='lanczos')
            packed = engine.render_crops(pic.dev, boxes, **kw)
            got = engine.render_crops(dev, boxes, layout=L, **kw)
            assert torch.equal(got, packed), (bw, bh, out_fmt, bgr)
        _check_all_sinks(engine, pic, bw, bh, oh, ow, frames=dev, layout=L)


def _offset_by_one(a):
    """The array's bytes on the device one byte behind an aligned address."""
    raw = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), a.ravel()])).cuda()
    return raw[1:].view(a.shape)


@pytest.mark.parametrize('pix_fmt', ops.PIX_FMTS)
def test_unaligned_buffers(engine, pictures, pix_fmt):
    """frames and out one byte off 16-alignment: the bytewise staging, every output row at another phase; the same bytes, and
    nothing written around the output."""
    pic = pictures[pix_fmt]
    (bw, bh), (oh, ow) = SHAPES[0]
    boxes, exp = pic.boxes(bw, bh), pic.expect(bw, bh, oh, ow)
    d = _offset_by_one(pic.fed)
    for out_fmt, bgr, want in (('rgb24', False, exp), ('rgb24', True, exp[..., ::-1]), ('nv12', False, forward(exp))):
        raw = torch.full((1 + want.size + 1,), 0x5A, dtype=torch.uint8, device='cuda')
        out = raw[1:-1].view(want.shape)
        assert d.data_ptr() % 16 == 1 and out.data_ptr() % 16 == 1
        got = engine.render_crops(d, boxes, out_hw=(oh, ow), bgr=bgr, out=out, pix_fmt=pix_fmt, out_fmt=out_fmt, interp='lanczos')
        assert np.array_equal(got.cpu().numpy(), want), (out_fmt, bgr)
        assert raw[0].item() == 0x5A and raw[-1].item() == 0x5A


def test_linear_through_the_new_entry_is_the_existing_entry(engine, pictures):
    """SVC_FILTER_LINEAR forwards: one copy case and one resize case, byte for byte the existing entry's."""
    pic = pictures['rgb24']
    lib = engine.lib
    lay = ops.frame_layout('rgb24', H, W).struct()
    for (bw, bh), (oh, ow) in (((101, 180), (180, 101)), ((101, 180), (320, 180))):
        boxes = torch.from_numpy(pic.boxes(bw, bh)).cuda()
        want = engine.render_crops(pic.dev, boxes, out_hw=(oh, ow))
        got = torch.zeros_like(want)
        rc = lib.svc_render_crops_filter(engine._h, pic.dev.data_ptr(), ctypes.byref(lay), N, H, W, boxes.data_ptr(), bw, bh,
                                         got.data_ptr(), _lib.FMT_RGB24, oh, ow, _lib.FILTER_LINEAR, 0, None)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(got, want), (bw, bh, oh, ow)
    # the window size with the Lanczos filter: both passes skipped, the existing exact copy
    boxes = pic.boxes(101, 180)
    got = engine.render_crops(pic.dev, boxes, interp='lanczos')
    assert torch.equal(got, engine.render_crops(pic.dev, boxes))
    assert engine.render_crops(pic.dev[:0], np.zeros((0, 4), np.int32), out_hw=(9, 9), interp='lanczos').shape == (0, 9, 9, 3)


def _lds_bytes(bw, bh, oh, ow, B=1):
    """include/svc.h's formula for an RGB output and a band of B rows."""
    up16 = lambda v: (v + 15) // 16 * 16
    vb = lanczos_ref.precompute_coeffs(bh, oh)[0].astype(int)
    T = max((vb[y0:y0 + B, 0] + vb[y0:y0 + B, 1]).max() - vb[y0:y0 + B, 0].min() for y0 in range(0, oh, B))
    return 2 * up16(3 * bw + 32) + T * up16(3 * ow) + 3 * ow + 16


def test_window_over_the_lds_budget_is_refused_and_the_largest_that_fits_renders(engine, pictures):
    """A 640 x 90 window to 180 rows: the vertical filters of one output row touch 6 window rows, so the smallest band needs
    2 * 1952 + 6 * 3 ow + 3 ow + 16 bytes: 71 120 for ow = 3200 (refused, nothing launched), 62 720 for ow = 2800 (a band of one row)."""
    pic = pictures['rgb24']
    bw, bh, oh = 640, 90, 180
    boxes = pic.boxes(bw, bh)
    assert _lds_bytes(bw, bh, oh, 3200) == 71120 > 65536 >= _lds_bytes(bw, bh, oh, 2800) == 62720 and _lds_bytes(bw, bh, oh, 2800, 2) > 65536
    out = torch.full((N, oh, 3200, 3), 7, dtype=torch.uint8, device='cuda')
    engine.profile_enable('render')
    with pytest.raises(_lib.SvcError, match=r'svc_render_crops_filter: window 640x90 -> 3200x180 \(lanczos\) needs 71120 bytes of LDS'):
        engine.render_crops(pic.dev, boxes, out_hw=(oh, 3200), out=out, interp='lanczos')
    assert engine.profile_read()[1] == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    got = engine.render_crops(pic.dev[:2], boxes[:2], out_hw=(oh, 2800), interp='lanczos')
    assert engine.profile_read()[1] == 1                          # counted under SVC_K_RENDER
    engine.profile_enable(None)
    assert np.array_equal(got.cpu().numpy(), _expect(pic.rgb[:2], boxes[:2], oh, 2800))


def test_render_video_every_container(engine):
    n, h, w, bw, bh, ow, oh = 45, 360, 640, 121, 360, 90, 200
    VD = dict(fc=n, bbs_np=_boxes(n, h, w, bw, bh, seed=5).astype(np.int64))
    lazy = synth.LazyBlobVideo(n + 3, h, w, seed=4)
    frames = lazy.select(range(n + 3)).cpu().numpy()
    exp = _expect(frames[:n], VD['bbs_np'], oh, ow)
    pinned = torch.from_numpy(frames).pin_memory()
    for name, cont in (('numpy', frames), ('pinned', pinned), ('cuda', torch.from_numpy(frames).cuda()), ('lazy', lazy)):
        got = render.render_video(cont, VD, engine=engine, out_size=(ow, oh), chunk=16, interp='lanczos')
        assert np.array_equal(got, exp), name
        seen = []
        render.render_video(dict(frames=cont), VD, engine=engine, out_size=(ow, oh), chunk=16, interp='lanczos',
                            sink=lambda c: seen.append(c.copy()))
        assert [len(c) for c in seen] == [16, 16, 13] and np.array_equal(np.concatenate(seen), exp), name
    got = render.render_video(frames, VD, engine=engine, out_size=(ow, oh), chunk=16, out_fmt='nv12', interp='lanczos')
    assert np.array_equal(got, forward(exp))


@pytest.mark.parametrize('out_pix_fmt', ('rgb24', 'nv12'))
def test_smart_vid_crop_writes_lanczos_frames(engine, tmp_path, out_pix_fmt):
    torch.set_num_threads(8)
    n, h, w = 40, 360, 640
    frames = synth.blob_frames(n, h, w, seed=4)
    video = dict(fr=30.0, frame_count=n, w=w, h=h, trans_inds=[0, n], frames=frames)
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    path = str(tmp_path / ('clip.' + out_pix_fmt))
    S.set_video_writer(ingest.write_frames_raw)
    try:
        VD, res = S.smart_vid_crop(video, CP, final_vid_fn=path, out_size=(100, 300), out_pix_fmt=out_pix_fmt, out_interp='lanczos',
                                   engine=engine)
    finally:
        S.set_video_writer(None)
    assert 't_render' in res
    exp = _expect(frames, VD['bbs_np'], 300, 100)
    if out_pix_fmt == 'nv12':
        exp = forward(exp)
    with open(path, 'rb') as fp:
        assert fp.read() == exp.tobytes()


def test_against_the_live_pillow(engine, pictures):
    Image = pytest.importorskip('PIL.Image')
    pic = pictures['rgb24']
    (bw, bh), (oh, ow) = SHAPES[2]
    boxes = pic.boxes(bw, bh)
    got = engine.render_crops(pic.dev, boxes, out_hw=(oh, ow), interp='lanczos').cpu().numpy()
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        want = np.asarray(Image.fromarray(np.ascontiguousarray(pic.rgb[i, y1:y2, x1:x2])).resize((ow, oh), Image.LANCZOS))
        assert np.array_equal(got[i], want), i
