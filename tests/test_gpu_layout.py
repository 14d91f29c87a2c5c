"""-m gpu: frames in a decoder's layout (svc_resize_frames_layout, svc_render_crops_layout and every door that takes a video
dict with layout=) against the PACKED entries on the packed copy of the same pictures, bit for bit.  No expected value is
computed here: each one is what the existing packed entry writes; nothing has a tolerance.  Pictures 36 x 64 and 38 x 66, n = 3."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import nv12_ref
from retargetvid_amd import _lib, ops, render, smartVidCrop as S, synth, weights

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

N = 3
PICTURES = ((36, 64), (38, 66))
SMALL = (20, 36)                                   # the down-scale's output (rows, columns)
# (bw, bh) -> the renders of that window: (out_hw or None for the copy, bgr, out_fmt)
WINDOWS = (((33, 21), ((None, False, 'rgb24'), (None, True, 'rgb24'),          # >= 16 wide, 16-groups run into the next window row
                       ((40, 50), False, 'rgb24'), ((40, 50), True, 'rgb24'), ((40, 50), False, 'nv12'),          # one resize up
                       ((10, 16), False, 'rgb24'), ((10, 16), True, 'rgb24'), ((10, 16), False, 'nv12'))),        # one resize down
           ((32, 20), ((None, False, 'rgb24'), (None, False, 'nv12'))),        # the NV12 sink's vector kernel, full strips
           ((24, 10), ((None, True, 'rgb24'), (None, False, 'nv12'))),         # ... and its half strip
           ((8, 8), ((None, False, 'rgb24'), (None, False, 'nv12'))),          # 8 wide: the per-pixel kernel
           ((1, 3), ((None, False, 'rgb24'),)),
           ((2, 2), ((None, True, 'rgb24'), (None, False, 'nv12'))),
           (('w', 'h'), ((None, False, 'rgb24'), (None, False, 'nv12'))))      # the whole picture: every row's last group runs on


def _boxes(h, w, bw, bh):
    """frame 0: the origin (row 0 of frame 0 is the first byte of the buffer); frame 1: the right and bottom edge; frame 2: an
    odd origin in x and y where the window leaves room."""
    xs = (0, w - bw, min(5, w - bw))
    ys = (0, h - bh, min(3, h - bh))
    return np.array([[x, y, x + bw, y + bh] for x, y in zip(xs, ys)], np.int32)


def _cases(h, w):
    for (bw, bh), renders in WINDOWS:
        bw, bh = (w, h) if bw == 'w' else (bw, bh)
        for out_hw, bgr, out_fmt in renders:
            yield bw, bh, out_hw, bgr, out_fmt


def _pictures(fmt, h, w, seed):
    shape = (N,) + ops.frame_shape(fmt, h, w)
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _pitch(packed, fmt, h, w, pitch, coded_h=None, chroma_pitch=None, gap=0, base=0, fill=0, n_tail=None):
    """The packed pictures laid out with these strides in a host buffer full of `fill` -> (buffer, FrameLayout).  The buffer
    ends with the last frame's last plane row (n_tail: bytes behind it, for containers that are [n, frame_stride])."""
    n = packed.shape[0]
    lay = dict(pitch=pitch)
    if fmt == 'nv12':
        lay.update(chroma_offset=pitch * (coded_h or h), chroma_pitch=chroma_pitch or pitch)
    L = ops.frame_layout(fmt, h, w, lay)
    L = ops.frame_layout(fmt, h, w, lay, L.extent + gap)
    buf = np.full(base + (n - 1) * L.frame_stride + L.extent + (L.frame_stride - L.extent if n_tail else 0), fill, np.uint8)
    view = np.lib.stride_tricks.as_strided
    if fmt == 'nv12':
        view(buf[base:], (n, h, w), (L.frame_stride, L.pitch, 1))[...] = packed[:, :h]
        view(buf[base + L.chroma_offset:], (n, h // 2, w), (L.frame_stride, L.chroma_pitch, 1))[...] = packed[:, h:]
    else:
        view(buf[base:], (n, h, 3 * w), (L.frame_stride, L.pitch, 1))[...] = packed.reshape(n, h, 3 * w)
    return buf, L


def _grid(fmt, h, w):
    """Every pairing of pitch x (coded height x chroma pitch) x frame gap x base the issue lists."""
    row = w if fmt == 'nv12' else 3 * w
    pitches = (row, row + 1, row + 3, row + 16, (row + 255) // 256 * 256)
    planes = [(ch, same) for ch in (h, h + 1, h + 6) for same in (True, False)] if fmt == 'nv12' else [(None, True)]
    for pitch, (ch, same), gap, base in itertools.product(pitches, planes, (0, 5, 4096), (0, 1, 8)):
        yield dict(pitch=pitch, coded_h=ch, chroma_pitch=pitch if same else pitch + 6, gap=gap, base=base)
    if fmt == 'nv12':
        # beside the issue's grid: an ODD luma pitch on the 16-byte paths.  In the grid an odd pitch brings an odd chroma_pitch,
        # which takes the byte paths; here chroma_offset (odd pitch x even coded height), chroma_pitch and frame_stride are even
        # and the buffer is 16-aligned, so px16 loads its luma bytes from odd addresses.
        for pitch, ch, gap in ((row + 1, h, 0), (row + 3, h + 6, 4096), (row + 17, h + 2, 2)):
            point = dict(pitch=pitch, coded_h=ch, chroma_pitch=row + 6, gap=gap, base=0)
            L = _pitch(np.zeros((1, h * 3 // 2, w), np.uint8), fmt, h, w, **point)[1]
            assert L.pitch % 2 == 1 and not (L.chroma_offset | L.chroma_pitch | L.frame_stride) % 2
            yield point


class _Plan:
    """All launches of one picture: the packed entries' results once (`exp`), the same launches on a pitched buffer (`run`)
    into a buffer of the same shape.  Every result lies on 256 bytes, so the 16-byte paths run whenever the input allows."""

    def __init__(self, engine, fmt, h, w, seed):
        self.engine, self.fmt, self.h, self.w = engine, fmt, h, w
        self.packed = _pictures(fmt, h, w, seed)
        self.items, off = [], 0
        shapes = [('small', (N,) + SMALL + (3,))]
        for bw, bh, out_hw, bgr, out_fmt in _cases(h, w):
            oh, ow = out_hw or (bh, bw)
            shapes.append(((bw, bh, bgr, out_fmt), (N,) + ops.out_frame_shape(out_fmt, oh, ow, bgr)))
        for what, shape in shapes:
            self.items.append((what, shape, off))
            off += (int(np.prod(shape)) + 255) // 256 * 256
        self.size = off
        self.boxes = {(bw, bh): torch.from_numpy(_boxes(h, w, bw, bh)).cuda() for bw, bh, _, _, _ in _cases(h, w)}
        self.exp = self.run(torch.from_numpy(self.packed).cuda(), None)
        torch.cuda.synchronize()

    def run(self, frames, layout):
        out = torch.full((self.size,), 0x5A, dtype=torch.uint8, device='cuda')
        for what, shape, off in self.items:
            dst = out[off:off + int(np.prod(shape))].view(shape)
            if what == 'small':
                dst.copy_(self.engine.resize_frames(frames, SMALL[0], SMALL[1], self.fmt, layout))
            else:
                bw, bh, bgr, out_fmt = what
                self.engine._render(frames, self.boxes[bw, bh], bw, bh, dst, bgr, self.fmt, out_fmt, layout)
        return out

    def check(self, got, where):
        if torch.equal(got, self.exp):
            return
        for what, shape, off in self.items:
            k = int(np.prod(shape))
            assert torch.equal(got[off:off + k], self.exp[off:off + k]), (self.fmt, self.h, self.w, what, shape, where)
        raise AssertionError(('bytes between the results changed', where))

    def on_device(self, buf, L, base):
        """The host buffer on the device as the [n, extent] view whose rows lie frame_stride apart: it ends where the buffer
        ends, nothing behind the last frame's extent belongs to it."""
        dev = torch.from_numpy(buf).cuda()
        assert dev.data_ptr() % 16 == 0
        return torch.as_strided(dev, (N, L.extent), (L.frame_stride, 1), base)


@pytest.fixture(scope='module')
def plans(engine):
    return {(fmt, h, w): _Plan(engine, fmt, h, w, seed=h + len(fmt)) for fmt in ops.PIX_FMTS for h, w in PICTURES}


@pytest.mark.parametrize('fmt', ops.PIX_FMTS)
@pytest.mark.parametrize('hw', PICTURES)
def test_grid_of_layouts_equals_the_packed_entries(plans, fmt, hw):
    """The down-scale and every render case on every layout of the grid, once with every padding byte 0x00 and once with
    0xFF: the packed entries' bytes both times, so no padding byte reaches a result."""
    plan = plans[(fmt,) + hw]
    h, w = hw
    points = list(_grid(fmt, h, w))
    assert len(points) == (270 + 3 if fmt == 'nv12' else 45)
    for point in points:
        for fill in (0x00, 0xFF):
            buf, L = _pitch(plan.packed, fmt, h, w, fill=fill, **point)
            assert buf.size == point['base'] + (N - 1) * L.frame_stride + L.extent
            plan.check(plan.run(plan.on_device(buf, L, point['base']), L), (point, fill))


@pytest.mark.parametrize('fmt', ops.PIX_FMTS)
def test_packed_layout_through_the_new_entries(plans, fmt):
    """The legacy entries are the packed layout of the same launchers: the layout entries on packed frames give their bytes."""
    for h, w in PICTURES:
        plan = plans[fmt, h, w]
        L = ops.frame_layout(fmt, h, w)
        assert L.frame_stride == plan.packed[0].size
        flat = torch.from_numpy(plan.packed).cuda().view(N, -1)
        plan.check(plan.run(flat, L), 'packed')
        plan.check(plan.run(flat, ops.frame_layout(fmt, h, w, None, L.frame_stride)), 'packed, explicit stride')


def test_engine_refuses_a_tensor_that_does_not_hold_the_layout(engine):
    L = ops.frame_layout('nv12', 36, 64, dict(pitch=128, chroma_offset=128 * 48), 9216)
    good = torch.zeros((2, 9216), dtype=torch.uint8, device='cuda')
    assert engine.resize_frames(good, 14, 25, 'nv12', L).shape == (2, 14, 25, 3)
    for bad in (torch.zeros((2, 9216 + 16), dtype=torch.uint8, device='cuda'),          # rows another stride apart
                torch.zeros((2, 72, 128), dtype=torch.uint8, device='cuda'),              # not 2-D
                good[:, :L.extent - 1],                                                   # rows shorter than a frame
                torch.zeros((2, 9216, 2), dtype=torch.uint8, device='cuda')[:, :, 0]):    # elements not adjacent
        with pytest.raises(ValueError):
            engine.resize_frames(bad, 14, 25, 'nv12', L)
        with pytest.raises(ValueError):
            engine.render_crops(bad, np.array([[0, 0, 16, 16]] * 2, np.int32), pix_fmt='nv12', layout=L)
    with pytest.raises(ValueError):
        engine.resize_frames(good, 14, 25, 'rgb24', L)                                    # the layout is one of NV12 frames
    with pytest.raises(TypeError):
        engine.resize_frames(good, 14, 25, 'nv12', dict(pitch=128))
    with pytest.raises(TypeError):
        engine.resize_frames(good.cpu(), 14, 25, 'nv12', L)


def test_c_abi_refuses_every_broken_rule(engine):
    """Through the library with a live handle and real buffers: SVC_E_INVALID with the rule, for both entries, and nothing is
    launched (the output keeps its bytes)."""
    lib, h, w = engine.lib, 36, 64
    frames = torch.zeros((2, 9216), dtype=torch.uint8, device='cuda')
    small = torch.full((2, 14, 25, 3), 7, dtype=torch.uint8, device='cuda')
    crops = torch.full((2, 16, 16, 3), 7, dtype=torch.uint8, device='cuda')
    boxes = torch.tensor([[0, 0, 16, 16]] * 2, dtype=torch.int32, device='cuda')
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def both(lay, out_fmt=0, flags=0, height=h, width=w):
        ref = ctypes.byref(lay)
        a = lib.svc_resize_frames_layout(engine._h, vp(frames), ref, 2, height, width, vp(small), 14, 25, None)
        ma = lib.svc_last_error().decode() if a else ''
        b = lib.svc_render_crops_layout(engine._h, vp(frames), ref, 2, height, width, vp(boxes), 16, 16, vp(crops), out_fmt, 16, 16, flags, None)
        mb = lib.svc_last_error().decode() if b else ''
        return a, ma, b, mb

    def st(fmt=1, stride=9216, pitch=128, coff=6144, cpitch=128, size=40):
        return _lib.SvcFrameLayout(size, fmt, stride, pitch, coff, cpitch)
    assert both(st())[::2] == (0, 0)
    torch.cuda.synchronize()
    small.fill_(7)
    crops.fill_(7)
    rgb_ext = 200 * 35 + 192
    for lay, text in ((st(pitch=63), "pitch 63 is below the row's 64 bytes"),
                      (st(fmt=0, stride=rgb_ext, pitch=191, coff=0, cpitch=0), "pitch 191 is below the row's 192 bytes"),
                      (st(cpitch=63), 'chroma_pitch 63 is below the width 64'),
                      (st(coff=128 * 35 + 63), 'the chroma plane overlaps the last luma row'),
                      (st(stride=6144 + 128 * 17 + 63), "frame_stride 8383 is below the frame's extent of 8384 bytes"),
                      (st(fmt=0, stride=rgb_ext - 1, pitch=200, coff=0, cpitch=0), "frame_stride 7191 is below the frame's extent of 7192 bytes"),
                      (st(stride=-9216), 'layout values must be non-negative'),
                      (st(cpitch=-128), 'layout values must be non-negative'),
                      (st(fmt=0, stride=rgb_ext, pitch=200, coff=7000, cpitch=200), 'chroma_offset and chroma_pitch must be 0 for rgb24'),
                      (st(size=32), 'struct_size is 32'),
                      (st(size=48), 'struct_size is 48'),
                      (st(fmt=2), 'unknown pix_fmt 2'),
                      (st(fmt=-1), 'unknown pix_fmt -1')):
        a, ma, b, mb = both(lay)
        assert a == b == -1 and text in ma and text in mb, (text, ma, mb)
        assert ma.startswith('svc_resize_frames_layout: ') and mb.startswith('svc_render_crops_layout: ')
    a, ma, b, mb = both(st(), out_fmt=2)
    assert (a, b) == (0, -1) and 'unknown out_fmt 2' in mb
    a, ma, b, mb = both(st(), out_fmt=1, flags=ops.RENDER_BGR)                  # what the packed _to_nv12 entries refuse
    assert (a, b) == (0, -1) and 'flags must be 0' in mb
    a, ma, b, mb = both(st(), flags=2)
    assert (a, b) == (0, -1) and 'SVC_RENDER_BGR' in mb
    a, ma, b, mb = both(st(), height=35)
    assert a == b == -1 and 'even' in ma and 'even' in mb
    assert lib.svc_resize_frames_layout(engine._h, vp(frames), None, 2, h, w, vp(small), 14, 25, None) == -1
    assert lib.svc_resize_frames_layout(engine._h, None, ctypes.byref(st()), 0, h, w, None, 14, 25, None) == 0       # n = 0: a no-op
    torch.cuda.synchronize()
    assert bool((crops == 7).all())
    engine.profile_enable('resize')
    L = ops.frame_layout('nv12', h, w, dict(pitch=128, chroma_offset=6144), 9216)
    engine.resize_frames(frames, 14, 25, 'nv12', L)
    assert engine.profile_read()[1] == 1                       # counted under SVC_K_RESIZE
    engine.profile_enable('render')
    engine.render_crops(frames, boxes, pix_fmt='nv12', layout=L)
    assert engine.profile_read()[1] == 1                       # ... and SVC_K_RENDER
    engine.profile_enable(None)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _videos(trans=(0, 15, 30), n=30, h=36, w=64, pitch=128, coded_h=48, seed=3, cut=15, fr=30.0):
    """A 2-shot video as packed NV12 and as a decoder would hand it out (30 frames of 64 x 36 at pitch 128, coded height 48):
    uint8 [n, pitch * coded_h * 3 / 2], every padding byte 0xFF."""
    rgb = synth.blob_frames(n, h, w, seed=seed)
    rgb[cut:] = rgb[cut:][:, ::-1]                              # a hard cut
    nv = nv12_ref.rgb_to_nv12(rgb)
    base = dict(fr=fr, frame_count=n, w=w, h=h, pix_fmt='nv12')
    if trans is not None:
        base['trans_inds'] = list(trans)
    stride = pitch * coded_h * 3 // 2
    buf, L = _pitch(nv, 'nv12', h, w, pitch=pitch, coded_h=coded_h, gap=stride - (pitch * coded_h + pitch * (h // 2 - 1) + w), fill=0xFF,
                    n_tail=True)
    assert L.frame_stride == stride and buf.size == n * stride
    return dict(base, frames=nv), dict(base, frames=buf.reshape(n, stride), layout=dict(pitch=pitch, chroma_offset=pitch * coded_h))


def _same(a, b):
    assert np.array_equal(a['smaps'], b['smaps'])
    assert a['dx'] == b['dx'] and a['dy'] == b['dy']
    assert np.array_equal(a['bbs_np'], b['bbs_np']) and a['true_inds'] == b['true_inds']


def _containers(video):
    f = video['frames']
    return (('numpy', video), ('cuda', dict(video, frames=torch.from_numpy(f).cuda())),
            ('pinned', dict(video, frames=torch.from_numpy(f).pin_memory())))


def test_end_to_end_equals_the_packed_video(engine, synthetic_sd):
    torch.set_num_threads(8)
    packed, pitched = _videos()
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    want, _ = S.smart_vid_crop(packed, CP, save_vid=False, engine=engine)
    assert want['smaps'].any()
    for name, video in _containers(pitched):
        got, _ = S.smart_vid_crop(video, CP, save_vid=False, engine=engine)
        _same(got, want)
    want_s, _ = S.smart_vid_crop(packed, CP, save_vid=False, engine=engine, stream_batch=16)
    got, _ = S.smart_vid_crop(pitched, CP, save_vid=False, engine=engine, stream_batch=16)
    _same(got, want_s)
    # the renderer: copy, a fixed size as BGR, NV12 out -- from every container
    for kw in (dict(), dict(out_size=(50, 40), bgr=True), dict(out_size=(50, 40), out_fmt='nv12')):
        exp = render.render_video(packed, want, engine=engine, chunk=16, **kw)
        for name, video in _containers(pitched):
            assert np.array_equal(render.render_video(video, want, engine=engine, chunk=16, **kw), exp), (name, kw)
        L = S.video_layout(pitched)
        assert np.array_equal(render.render_video(pitched['frames'], want, engine=engine, layout=L, **kw), exp)
    # the scheduler: pitched host, pitched device and packed videos in one job
    vids = [pitched, _containers(pitched)[1][1], packed]
    par = S.crop_videos(vids, CP, ('1:3', '3:1'), workers=1, state_dict=synthetic_sd)
    twins = S.crop_videos([packed] * 3, CP, ('1:3', '3:1'), workers=1, state_dict=synthetic_sd)
    for p, t in zip(par, twins):
        for r in ('1:3', '3:1'):
            assert np.array_equal(p[r][0]['bbs_np'], t[r][0]['bbs_np']) and np.array_equal(p[r][0]['smaps'], t[r][0]['smaps'])
            assert p[r][0]['dx'] == t[r][0]['dx']
    assert np.array_equal(par[0]['1:3'][0]['bbs_np'], want['bbs_np'])


def test_selected_frames_of_a_device_container_are_read_where_they_lie(engine):
    """FrameSource.small on a CUDA container: consecutive frames, every k-th frame (one strided view, frames k surfaces apart) and
    an irregular selection (cut into such runs) give the packed container's bytes, and nothing is gathered: the down-scale is
    handed views of the container itself."""
    packed, pitched = _videos()
    L = S.video_layout(pitched)
    d_packed, d_pitched = torch.from_numpy(packed['frames']).cuda(), torch.from_numpy(pitched['frames']).cuda()
    lo, hi = d_pitched.data_ptr(), d_pitched.data_ptr() + d_pitched.numel()
    seen = []
    real = engine.resize_frames

    def spy(frames, *a, **k):
        seen.append(lo <= frames.data_ptr() < hi)
        return real(frames, *a, **k)
    for idx in (list(range(4, 20)), list(range(1, 30, 6)), [0], [29], [0, 1, 2, 7, 12, 17, 18, 29], [5, 3, 1], [2, 2, 9]):
        want = S.FrameSource.of(d_packed, 'nv12').small(engine, idx, 140, 250)
        engine.resize_frames = spy
        try:
            got = S.FrameSource.of(d_pitched, 'nv12', L).small(engine, idx, 140, 250)
        finally:
            del engine.resize_frames
        assert got.shape == want.shape and torch.equal(got, want), idx
    assert seen and all(seen)


def test_stream_pipeline_takes_frames_with_a_layout(engine):
    """StreamPipeline.submit_frames(layout=): the maps and centres of the packed frames."""
    from retargetvid_amd import pipeline
    packed, pitched = _videos()
    CP = S.sc_init_crop_params()
    L = S.video_layout(pitched)
    out = []
    for frames, layout in ((packed['frames'], None), (pitched['frames'], L)):
        maps = torch.zeros((8, 140, 250), dtype=torch.uint8, device='cuda')
        pipe = pipeline.StreamPipeline(engine, CP, 140, 250, batch=8, maps_out=maps)
        pipe.submit_frames(torch.from_numpy(frames[8:16]).cuda(), np.zeros(8, np.uint8), pix_fmt='nv12', layout=layout)
        xy = np.array(sorted(pipe.finish()), np.float64)
        torch.cuda.synchronize()
        out.append((maps.cpu().numpy(), xy))
    assert out[0][0].any() and len(out[0][1]) == 8
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1], equal_nan=True)


def test_shot_detection_sees_equal_bytes(engine):
    """tests/test_gpu_nv12.py's shot video (150 frames of 160 x 90, a cut at 60: these weights give it scenes from frame 0) as
    surfaces of pitch 256 and coded height 96: detect_shots, and the ingest that runs it from the plan, see the packed bytes."""
    from retargetvid_amd import transnetv1_handler as Hd
    net = Hd.ShotTransNet(Hd.ShotTransNetParams(), weights=weights.make_transnet_state_dict(0))
    try:
        packed, pitched = _videos(trans=None, n=150, h=90, w=160, pitch=256, coded_h=96, seed=9, cut=60, fr=25.0)
        CP = dict(S.sc_init_crop_params(), read_batch=64, out_ratio='1:3', hdbscan_min=5)
        want = S.detect_shots(packed['frames'], 25.0, CP, net=net, pix_fmt='nv12')
        L = S.video_layout(pitched)
        for name, video in _containers(pitched):
            got = S.detect_shots(video['frames'], 25.0, CP, net=net, pix_fmt='nv12', layout=L)
            assert np.array_equal(got['trans_probs'], want['trans_probs']) and np.array_equal(got['segmentation'], want['segmentation']), name
        full, _ = S.smart_vid_crop(packed, CP, save_vid=False, engine=engine, shot_net=net)      # a result, not a refusal
        assert full['smaps'].any() and len(full['trans_probs']) == 150
        for name, video in _containers(pitched)[:2]:
            got, _ = S.smart_vid_crop(video, CP, save_vid=False, engine=engine, shot_net=net)
            assert np.array_equal(got['trans_probs'], full['trans_probs']), name
            _same(got, full)
    finally:
        net.close()
