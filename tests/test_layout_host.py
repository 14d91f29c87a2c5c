"""Frame layouts on the host (no GPU): the rules of ops.frame_layout (the ones include/svc.h states and the C launchers
check), the packed layout of each format, and the layout's way through the video dict -- video_pix_fmt / video_layout,
plan_video, the render door's container check and the feature cache's key -- before any device work."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from retargetvid_amd import _lib, ops, render, smartVidCrop as S
from retargetvid_amd.frames import FrameSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 36, 64


def _nv12_dict(frame_stride=128 * 48 * 3 // 2, n=4, **layout):
    layout = dict(dict(pitch=128, chroma_offset=128 * 48), **layout)
    return dict(frames=np.zeros((n, frame_stride), np.uint8), fr=25.0, frame_count=n, w=W, h=H, pix_fmt='nv12', layout=layout,
                trans_inds=[0, n])


@pytest.mark.parametrize('fmt,layout,stride,text', [
    ('rgb24', dict(pitch=3 * W - 1), None, "pitch 191 is below the row's 192 bytes"),                    # pitch one byte short
    ('nv12', dict(pitch=W - 1), None, "pitch 63 is below the row's 64 bytes"),
    ('nv12', dict(pitch=128, chroma_pitch=W - 1), None, 'chroma_pitch 63 is below the width 64'),
    ('nv12', dict(pitch=128, chroma_offset=128 * (H - 1) + W - 1), None, 'the chroma plane overlaps the last luma row'),
    ('nv12', dict(pitch=128, chroma_offset=128 * 48), 128 * 48 + 128 * 17 + W - 1, "frame_stride 8383 is below the frame's extent of 8384 bytes"),
    ('rgb24', dict(pitch=200), 200 * (H - 1) + 3 * W - 1, "frame_stride 7191 is below the frame's extent of 7192 bytes"),   # one byte short
    ('nv12', dict(pitch=-128), None, 'layout values must be non-negative'),
    ('nv12', dict(pitch=128, chroma_offset=-1), None, 'layout values must be non-negative'),
    ('rgb24', dict(pitch=200), -1, 'layout values must be non-negative'),
    ('rgb24', dict(pitch=200, chroma_pitch=200), None, 'chroma_offset and chroma_pitch must be 0 for rgb24'),
    ('rgb24', dict(chroma_offset=7000), None, 'chroma_offset and chroma_pitch must be 0 for rgb24'),
    ('nv12', dict(stride=128), None, "unknown layout key 'stride'"),
])
def test_every_rule_raises_with_its_text(fmt, layout, stride, text):
    with pytest.raises(ValueError) as e:
        ops.frame_layout(fmt, H, W, layout, stride)
    assert text in str(e.value)


def test_the_limits_themselves_are_legal():
    L = ops.frame_layout('nv12', H, W, dict(pitch=W, chroma_offset=W * (H - 1) + W, chroma_pitch=W), W * H * 3 // 2)
    assert L.extent == L.frame_stride == W * H * 3 // 2
    L = ops.frame_layout('nv12', H, W, dict(pitch=65, chroma_offset=65 * 35 + 64, chroma_pitch=67))      # odd values: no alignment is demanded
    assert L.extent == L.frame_stride == 65 * 35 + 64 + 67 * 17 + 64
    L = ops.frame_layout('rgb24', H, W, dict(pitch=193), 193 * 35 + 192)
    assert (L.chroma_offset, L.chroma_pitch, L.extent) == (0, 0, 193 * 35 + 192)
    with pytest.raises(ValueError):
        ops.frame_layout('nv12', H + 1, W, None)                 # the picture's own rules come first
    with pytest.raises(ValueError):
        ops.frame_layout('yuv420p', H, W, None)


@pytest.mark.parametrize('fmt', ops.PIX_FMTS)
def test_the_packed_layout_is_frame_shapes_byte_count(fmt):
    for h, w in ((H, W), (38, 66), (1080, 1920)):
        L = ops.frame_layout(fmt, h, w)
        nbytes = int(np.prod(ops.frame_shape(fmt, h, w)))
        assert L.frame_stride == L.extent == nbytes
        assert L.pitch == (w if fmt == 'nv12' else 3 * w)
        assert (L.chroma_offset, L.chroma_pitch) == ((w * h, w) if fmt == 'nv12' else (0, 0))
        assert L == ops.frame_layout(fmt, h, w, dict(pitch=None), nbytes)
    # a decoder's 1080p surface: missing keys follow the pitch
    L = ops.frame_layout('nv12', 1080, 1920, dict(pitch=2048, chroma_offset=2048 * 1088), 2048 * 1632)
    assert (L.chroma_pitch, L.extent, L.frame_stride) == (2048, 2048 * 1088 + 2048 * 539 + 1920, 2048 * 1632)


def test_every_kth_frame_is_a_layout_too():
    L = ops.frame_layout('nv12', H, W, dict(pitch=128, chroma_offset=6144), 9216)
    K = L.every(6)
    assert K.key() == ('nv12', H, W, 6 * 9216, 128, 6144, 128) and K.extent == L.extent and L.frame_stride == 9216
    assert K == ops.frame_layout('nv12', H, W, dict(pitch=128, chroma_offset=6144), 6 * 9216) and L.every(1) == L


@pytest.mark.parametrize('idx,runs', [
    ([], []),
    ([7], [(7, 1, 1)]),
    (list(range(4, 20)), [(4, 16, 1)]),                               # consecutive frames: one view
    (list(range(1, 30, 6)), [(1, 5, 6)]),                             # every skip-th frame: one strided view
    ([0, 1, 2, 7, 12, 17, 18, 29], [(0, 3, 1), (7, 3, 5), (18, 2, 11)]),       # greedy from the left
    ([0, 1, 2, 7, 12, 17, 18], [(0, 3, 1), (7, 3, 5), (18, 1, 1)]),
    ([5, 3, 1], [(5, 1, 1), (3, 1, 1), (1, 1, 1)]),                   # a step backwards continues no run
    ([2, 2, 9], [(2, 1, 1), (2, 2, 7)]),                              # nor does a repeat
    ([2, 2, 2], [(2, 1, 1), (2, 1, 1), (2, 1, 1)]),
    ([3, 9], [(3, 2, 6)]),
])
def test_a_selection_is_cut_into_strided_runs(idx, runs):
    """smartVidCrop._runs: what FrameSource.small reads from a device container, as views -- every run restores its frames in order."""
    assert S._runs(idx) == runs
    assert S._runs(np.array(idx, np.int64)) == runs
    frames = np.arange(40)
    got = [int(v) for first, count, step in runs for v in frames[first:first + (count - 1) * step + 1:step]]
    assert got == idx and all(count >= 1 and step >= 1 for _, count, step in runs)


def test_the_struct_is_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    body = re.search(r'typedef struct SvcFrameLayout \{(.*?)\} SvcFrameLayout;', hdr, flags=re.S).group(1)
    fields = re.findall(r'\b(u?int(?:32|64)_t)\s+(\w+);', body)
    ctype = dict(uint32_t=ctypes.c_uint32, int32_t=ctypes.c_int32, int64_t=ctypes.c_int64)
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.SvcFrameLayout._fields_)
    assert ctypes.sizeof(_lib.SvcFrameLayout) == 40
    assert (int(re.search(r'#define SVC_FMT_RGB24 (\d+)', hdr).group(1)), int(re.search(r'#define SVC_FMT_NV12\s+(\d+)', hdr).group(1))) \
        == (ops.PIX_FMTS.index('rgb24'), ops.PIX_FMTS.index('nv12')) == (_lib.FMT_RGB24, _lib.FMT_NV12) \
        == (ops.OUT_FMTS.index('rgb24'), ops.OUT_FMTS.index('nv12'))
    s = ops.frame_layout('nv12', H, W, dict(pitch=128, chroma_offset=128 * 48), 9221).struct()
    assert (s.struct_size, s.pix_fmt, s.frame_stride, s.pitch, s.chroma_offset, s.chroma_pitch) == (40, 1, 9221, 128, 6144, 128)


def test_abi_version_agrees_everywhere():
    hdr = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    assert int(re.search(r'#define SVC_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == _lib.load().svc_abi_version() == 13
    assert re.search(r'\* 12 = .*svc_resize_frames_layout.*svc_render_crops_layout', hdr)
    lib = _lib.load()
    assert hasattr(lib, 'svc_resize_frames_layout') and hasattr(lib, 'svc_render_crops_layout')


def test_the_launchers_refuse_a_bad_layout_without_a_device():
    """The argument checks come before any device work: they answer on a machine without a GPU, with the rule."""
    lib = _lib.load()

    def resize(lay, h=H, w=W):
        rc = lib.svc_resize_frames_layout(None, None, ctypes.byref(lay) if lay is not None else None, 0, h, w, None, 14, 25, None)
        return rc, lib.svc_last_error().decode()

    def st(fmt, stride, pitch, coff, cpitch, size=40):
        return _lib.SvcFrameLayout(size, fmt, stride, pitch, coff, cpitch)
    assert resize(None) == (-1, 'svc_resize_frames_layout: layout is NULL')
    rc, msg = resize(st(1, 9216, 128, 6144, 128, size=32))
    assert rc == -1 and 'struct_size is 32' in msg
    rc, msg = resize(st(2, 9216, 128, 6144, 128))
    assert rc == -1 and 'unknown pix_fmt 2' in msg
    rc, msg = resize(st(1, 9216, 63, 6144, 128))
    assert rc == -1 and "pitch 63 is below the row's 64 bytes" in msg
    rc, msg = resize(st(1, 9216, 128, 128 * 35 + 63, 128))
    assert rc == -1 and 'the chroma plane overlaps the last luma row' in msg
    rc, msg = resize(st(1, 9216, 128, 6144, 63))
    assert rc == -1 and 'chroma_pitch 63 is below the width 64' in msg
    rc, msg = resize(st(1, 8383, 128, 6144, 128))
    assert rc == -1 and "frame_stride 8383 is below the frame's extent of 8384 bytes" in msg
    rc, msg = resize(st(1, 9216, 128, -6144, 128))
    assert rc == -1 and 'layout values must be non-negative' in msg
    rc, msg = resize(st(0, 7192, 200, 0, 200))
    assert rc == -1 and 'chroma_offset and chroma_pitch must be 0 for rgb24' in msg
    rc, msg = resize(st(1, 2 ** 62, 2 ** 62, 2 ** 62, 128))              # a product past 2^63 fails its rule, it does not wrap past it
    assert rc == -1 and 'chroma_offset' in msg
    rc = lib.svc_resize_frames_layout(None, None, ctypes.byref(st(1, 2 ** 62, 128, 6144, 128)), 3, H, W, None, 14, 25, None)
    assert rc == -1 and '3 frames of frame_stride 4611686018427387904 span more than PTRDIFF_MAX bytes' in lib.svc_last_error().decode()
    rc, msg = resize(st(1, 9216, 128, 6144, 128), h=35)
    assert rc == -1 and 'even' in msg
    rc = lib.svc_render_crops_layout(None, None, ctypes.byref(st(1, 9216, 128, 6144, 128)), 0, H, W, None, 16, 16, None, 2, 16, 16, 0, None)
    assert rc == -1 and 'unknown out_fmt 2' in lib.svc_last_error().decode()


def _nhwf(src):
    return src.n, src.h, src.w, src.pix_fmt


def test_the_video_dict_carries_the_layout():
    v = _nv12_dict()
    assert S.video_pix_fmt(v) == 'nv12'
    L = S.video_layout(v)
    assert L == ops.frame_layout('nv12', H, W, dict(pitch=128, chroma_offset=6144, chroma_pitch=128), 9216)
    assert S.video_layout(dict(v, layout=None)) is None and S.video_layout({k: x for k, x in v.items() if k != 'layout'}) is None
    plan = S.plan_video(v, S.sc_init_crop_params())
    assert plan['source'].layout == L and plan['source'].pix_fmt == 'nv12' and (plan['h'], plan['w']) == (H, W)
    packed = dict(v, frames=np.zeros((4, 54, 64), np.uint8), layout=None)
    assert S.plan_video(packed, S.sc_init_crop_params())['source'].layout is None
    assert _nhwf(FrameSource.of(v)) == (4, H, W, 'nv12')
    assert FrameSource.of(v).layout == L
    rgb = dict(frames=np.zeros((4, 200 * H), np.uint8), fr=25.0, frame_count=4, w=W, h=H, layout=dict(pitch=200), trans_inds=[0, 4])
    assert S.video_pix_fmt(rgb) == 'rgb24' and S.plan_video(rgb, S.sc_init_crop_params())['source'].layout.pitch == 200
    assert _nhwf(FrameSource.of(rgb)) == (4, H, W, 'rgb24')


def test_the_video_dict_is_refused_before_any_device_work():
    for bad, text in ((_nv12_dict(pitch=63), "pitch 63 is below the row's 64 bytes"),
                      (_nv12_dict(chroma_offset=128 * 35 + 63), 'overlaps the last luma row'),
                      (_nv12_dict(frame_stride=8383), "frame_stride 8383 is below the frame's extent of 8384 bytes"),
                      (_nv12_dict(chroma_pitch=-128), 'non-negative'),
                      (dict(_nv12_dict(), frames=np.zeros((4, 54, 64), np.uint8)), 'are uint8 [n, frame_stride], not (4, 54, 64)'),
                      (dict(frames=np.zeros((4, 200 * H), np.uint8), fr=25.0, frame_count=4, w=W, h=H, trans_inds=[0, 4],
                            layout=dict(pitch=200, chroma_offset=200 * H, chroma_pitch=200)), 'must be 0 for rgb24')):
        for door in (S.video_pix_fmt, S.video_layout, lambda v: S.plan_video(v, S.sc_init_crop_params()), FrameSource.of,
                     lambda v: render.render_video(v, dict(fc=0, bbs_np=np.zeros((0, 4), np.int64)))):
            with pytest.raises(ValueError) as e:
                door(bad)
            assert text in str(e.value)

    class Gen:                                                   # an on-device generator: frames on demand, nothing to lay out
        h, w = H, W

        def __len__(self):
            return 4

        def select(self, idx):
            raise AssertionError('no frame may be asked for')
    for door in (S.video_pix_fmt, lambda v: S.plan_video(v, S.sc_init_crop_params()), FrameSource.of):
        with pytest.raises(ValueError) as e:
            door(dict(_nv12_dict(), frames=Gen()))
        assert '.select' in str(e.value)


def test_the_cache_key_differs_between_layouts(tmp_path):
    """smart_vid_crop's feature cache: its key names the layout, so a file written under one is not read back under another."""
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    eng = type('E', (), dict(weights_id=1))()
    a, b = _nv12_dict(), _nv12_dict(frame_stride=9216 + 64)
    c = _nv12_dict(frame_stride=160 * 48 * 3 // 2, pitch=160, chroma_offset=160 * 48)
    packed = dict(a, frames=np.zeros((4, 54, 64), np.uint8), layout=None)
    keys = [S.feature_cache_key(v, CP, eng) for v in (a, b, c, packed)]
    assert all(keys[i] != keys[j] for i in range(4) for j in range(i))
    assert keys[0] == S.feature_cache_key(_nv12_dict(), CP, eng)
    assert keys[0]['layout'] == S.video_layout(a).key() and keys[0]['pix_fmt'] == 'nv12'
    assert 'layout' not in keys[3]                               # a packed dict keeps the key it always had
    assert pickle.loads(pickle.dumps(keys[0])) == keys[0]        # it is stored beside the analysis
