"""Output layouts on the host (no GPU): svc_render_crops_to_layout in header, binding and EXPORTS; every rule of the C launcher for
out_layout, with its text and with the side named, and each limit itself legal (NULL handle: nothing is launched); the Python doors
-- Engine.render_crops, render.render_video, smart_vid_crop, ingest.write_frames_raw -- that refuse a mismatched or broken
out_layout before any device work and before a writer is opened; and the writer's layout= keyword, present only when one is given."""
import ctypes
import os
import re

import numpy as np
import pytest

from retargetvid_amd import _lib, ingest, ops, render, smartVidCrop as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 36, 64                       # the frames
OH, OW = 20, 30                     # the output picture
ENTRY = 'svc_render_crops_to_layout'


def _header():
    return open(os.path.join(ROOT, 'include', 'svc.h')).read()


def test_header_binding_and_exports_agree():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    proto = re.search(r'int\s+%s\s*\(([^)]*)\)\s*;' % ENTRY, text)
    assert proto, ENTRY + ' is not declared'
    params = [' '.join(p.split()) for p in proto.group(1).split(',')]
    assert params == ['SvcHandle *h', 'const uint8_t *frames', 'const SvcFrameLayout *layout', 'const SvcColour *in_colour', 'int n',
                      'int height', 'int width', 'const int32_t *boxes', 'int bw', 'int bh', 'uint8_t *out',
                      'const SvcFrameLayout *out_layout', 'const SvcColour *out_colour', 'int oh', 'int ow', 'int filter', 'int flags',
                      'void *stream']
    assert ENTRY in _lib.EXPORTS and _lib.EXPORTS.count(ENTRY) == 1
    lib = _lib.load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = [i32 if p.startswith('int ') else ctypes.POINTER(_lib.SvcFrameLayout) if 'SvcFrameLayout' in p
            else ctypes.POINTER(_lib.SvcColour) if 'SvcColour' in p else vp for p in params]
    fn = getattr(lib, ENTRY)
    assert fn.argtypes == want and fn.restype == i32


def test_abi_version_agrees_everywhere_and_the_history_names_the_entry():
    hdr = _header()
    assert int(re.search(r'#define SVC_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == _lib.load().svc_abi_version() == 13
    assert re.search(r'\* 12 = .*svc_resize_frames_layout.*svc_render_crops_layout', hdr)       # the line is not reshaped
    history = hdr[hdr.index('ABI revision of the loaded library'):hdr.index('#define SVC_ABI_VERSION')]
    assert ENTRY in history[history.index('(12, no bump)'):history.index(' * 13 = ')]      # the entry came under revision 12, without a bump
    assert ctypes.sizeof(_lib.SvcFrameLayout) == 40             # the struct is the one the frames' layout uses, unchanged


def _st(fmt, stride, pitch, coff, cpitch, size=40):
    return _lib.SvcFrameLayout(size, fmt, stride, pitch, coff, cpitch)


def _call(olay, oh=OH, ow=OW, n=0, out_colour=None, flags=0, filt=0, in_fmt='rgb24', h=None):
    """The entry with a NULL handle and n = 0: every answer is an argument check's, nothing can be launched."""
    lib = _lib.load()
    lay = ops.frame_layout(in_fmt, H, W).struct()
    rc = getattr(lib, ENTRY)(h, None, ctypes.byref(lay), None, n, H, W, None, 16, 16, None, ctypes.byref(olay) if olay is not None else None,
                             ctypes.byref(out_colour) if out_colour is not None else None, oh, ow, filt, flags, None)
    return rc, lib.svc_last_error().decode()


NV_PITCH, NV_CO, NV_CP = 40, 40 * 24, 48                        # a legal NV12 layout of the 30 x 20 output
NV_EXTENT = NV_CO + NV_CP * (OH // 2 - 1) + OW


@pytest.mark.parametrize('olay,text', [
    (_st(1, 4096, NV_PITCH, NV_CO, NV_CP, size=32), 'SvcFrameLayout.struct_size is 32'),                    # a stale binding
    (_st(2, 4096, NV_PITCH, NV_CO, NV_CP), 'unknown pix_fmt 2'),
    (_st(-1, 4096, NV_PITCH, NV_CO, NV_CP), 'unknown pix_fmt -1'),
    (_st(0, 4096, 3 * OW - 1, 0, 0), "pitch 89 is below the row's 90 bytes"),                                # one byte short
    (_st(1, 4096, OW - 1, NV_CO, NV_CP), "pitch 29 is below the row's 30 bytes"),
    (_st(1, 4096, NV_PITCH, NV_CO, OW - 1), 'chroma_pitch 29 is below the width 30'),
    (_st(1, 4096, NV_PITCH, NV_PITCH * (OH - 1) + OW - 1, NV_CP), 'the chroma plane overlaps the last luma row'),
    (_st(1, NV_EXTENT - 1, NV_PITCH, NV_CO, NV_CP), "frame_stride %d is below the frame's extent of %d bytes" % (NV_EXTENT - 1, NV_EXTENT)),
    (_st(0, 96 * (OH - 1) + 3 * OW - 1, 96, 0, 0), "frame_stride 1913 is below the frame's extent of 1914 bytes"),
    (_st(1, 4096, -NV_PITCH, NV_CO, NV_CP), 'layout values must be non-negative'),
    (_st(1, 4096, NV_PITCH, -1, NV_CP), 'layout values must be non-negative'),
    (_st(1, 4096, NV_PITCH, NV_CO, -NV_CP), 'layout values must be non-negative'),
    (_st(0, -1, 96, 0, 0), 'layout values must be non-negative'),
    (_st(0, 4096, 96, 0, 96), 'chroma_offset and chroma_pitch must be 0 for rgb24'),
    (_st(0, 4096, 96, 2000, 0), 'chroma_offset and chroma_pitch must be 0 for rgb24'),
    (_st(1, 2 ** 62, 2 ** 62, 2 ** 62, NV_CP), 'chroma_offset'),           # a product past 2^63 fails its rule, it does not wrap past it
])
def test_every_rule_of_the_launcher_raises_with_its_text_and_names_the_side(olay, text):
    rc, msg = _call(olay)
    assert rc == -1 and msg.startswith(ENTRY + ': out_layout: ') and text in msg


def test_the_other_refusals_of_the_launcher():
    rc, msg = _call(None)
    assert (rc, msg) == (-1, ENTRY + ': out_layout: layout is NULL')
    rc, msg = _call(_st(1, 2 ** 62, NV_PITCH, NV_CO, NV_CP), n=3)
    assert rc == -1 and 'out_layout: 3 frames of frame_stride 4611686018427387904 span more than PTRDIFF_MAX bytes' in msg
    # the picture's own rules are the sink's, in its words
    rc, msg = _call(_st(1, 4096, NV_PITCH, NV_CO, NV_CP), oh=OH + 1)
    assert rc == -1 and 'out_layout: an output of 30x21 (width and height of an NV12 output are even and >= 2' in msg
    rc, msg = _call(_st(0, 4096, 96, 0, 0), ow=0)
    assert rc == -1 and 'out_layout: an output of 0x20 (an RGB output has width and height >= 1)' in msg
    # the frames' own layout still answers without a side, the filter and the colours as in svc_render_crops_colour
    lib = _lib.load()
    bad_in = _st(0, 0, 3 * W - 1, 0, 0)
    ok_out = _st(0, 4096, 96, 0, 0)
    rc = getattr(lib, ENTRY)(None, None, ctypes.byref(bad_in), None, 0, H, W, None, 16, 16, None, ctypes.byref(ok_out), None, OH, OW, 0, 0, None)
    assert rc == -1 and lib.svc_last_error().decode() == ENTRY + ": pitch 191 is below the row's 192 bytes"
    rc, msg = _call(ok_out, filt=2)
    assert rc == -1 and msg == ENTRY + ': unknown filter 2 (SVC_FILTER_LINEAR or SVC_FILTER_LANCZOS)'
    col = _lib.SvcColour(ctypes.sizeof(_lib.SvcColour), 1, 1, 0)
    rc, msg = _call(ok_out, out_colour=col)                     # pix_fmt of out_layout takes the place of out_fmt
    assert rc == -1 and ENTRY + ': out_colour is given but that side is rgb24' in msg
    fake = ctypes.c_void_p(16)                                  # never dereferenced: the flags rule answers first (n = 0)
    rc, msg = _call(_st(1, 4096, NV_PITCH, NV_CO, NV_CP), flags=ops.RENDER_BGR, h=fake)
    assert rc == -1 and 'flags must be 0 (SVC_RENDER_BGR has no meaning for an NV12 output)' in msg


@pytest.mark.parametrize('olay,colour', [
    (_st(0, 3 * OW * OH, 3 * OW, 0, 0), False),                                              # the packed values
    (_st(0, 91 * (OH - 1) + 3 * OW, 91, 0, 0), False),                                       # an odd pitch, frame_stride = extent
    (_st(1, OW * OH * 3 // 2, OW, OW * OH, OW), True),                                       # packed NV12
    (_st(1, NV_EXTENT, NV_PITCH, NV_CO, NV_CP), True),                                       # frame_stride = extent
    (_st(1, 31 * (OH - 1) + OW + 33 * (OH // 2 - 1) + OW, 31, 31 * (OH - 1) + OW, 33), True),     # the chroma plane right behind the last luma row; odd values
    (_st(1, 2 ** 61, 2 ** 40, 2 ** 50, 2 ** 40), False),                                     # large and addressable (n = 0)
])
def test_the_limits_themselves_are_legal(olay, colour):
    """A legal out_layout passes every layout and colour check: the answer is the next check's, the NULL handle."""
    col = _lib.SvcColour(ctypes.sizeof(_lib.SvcColour), 1, 1, 0) if colour else None
    for filt in (0, 1):
        assert _call(olay, out_colour=col, filt=filt) == (-1, ENTRY + ': invalid argument')


# ---- the Python doors ---------------------------------------------------------------------------------------------------------------
def _video(n=4):
    return dict(frames=np.zeros((n, H, W, 3), np.uint8), fr=25.0, frame_count=n, w=W, h=H, trans_inds=[0, n])


def _vd(n=4, bw=OW, bh=OH):
    return dict(fc=n, bbs_np=np.array([[2, 4, 2 + bw, 4 + bh]] * n, np.int64))


BROKEN = [
    ('rgb24', dict(pitch=3 * OW - 1), "out_layout: pitch 89 is below the row's 90 bytes"),
    ('nv12', dict(pitch=OW - 1), "out_layout: pitch 29 is below the row's 30 bytes"),
    ('nv12', dict(pitch=40, chroma_pitch=29), 'out_layout: chroma_pitch 29 is below the width 30'),
    ('nv12', dict(pitch=40, chroma_offset=40 * 19 + 29), 'the chroma plane overlaps the last luma row'),
    ('nv12', dict(pitch=-40), 'out_layout: layout values must be non-negative'),
    ('rgb24', dict(pitch=96, chroma_pitch=96), 'out_layout: chroma_offset and chroma_pitch must be 0 for rgb24'),
    ('rgb24', dict(stride=96), "out_layout: unknown layout key 'stride'"),
    ('rgb24', 96, 'out_layout is an ops.FrameLayout or dict'),
]
MISMATCHED = [
    ('rgb24', ops.frame_layout('nv12', OH, OW, dict(pitch=64)), 'out_layout is one of nv12 frames'),
    ('nv12', ops.frame_layout('rgb24', OH, OW, dict(pitch=96)), 'out_layout is one of rgb24 frames'),
    ('rgb24', ops.frame_layout('rgb24', OH + 2, OW, dict(pitch=96)), 'out_layout is one of 30 x 22 pictures, the output is 30 x 20'),
    ('nv12', ops.frame_layout('nv12', OH, OW + 2, dict(pitch=64)), 'out_layout is one of 32 x 20 pictures, the output is 30 x 20'),
]


@pytest.mark.parametrize('fmt,lay,text', BROKEN + MISMATCHED)
def test_render_video_refuses_before_any_device_work(fmt, lay, text, monkeypatch):
    monkeypatch.setattr(S, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    for kw in (dict(), dict(out_size=(OW, OH))):                # the window's own size, and a resampled window of another
        vd = _vd() if not kw else _vd(bw=24, bh=16)
        with pytest.raises(ValueError) as e:
            render.render_video(_video(), vd, out_fmt=fmt, out_layout=lay, **kw)
        assert text in str(e.value)


def test_render_video_resolves_a_dict_against_the_final_size():
    """fc = 0 returns before the device: what comes back shows the resolved layout -- [0, frame_stride]."""
    vd = dict(fc=0, bbs_np=np.zeros((0, 4), np.int64))
    out = render.render_video(_video(), vd, out_size=(OW, OH), out_layout=dict(pitch=96))
    assert out.shape == (0, 96 * (OH - 1) + 3 * OW) and out.dtype == np.uint8
    out = render.render_video(_video(), vd, out_size=(OW, OH), out_fmt='nv12', out_layout=dict(pitch=64, chroma_offset=64 * 24))
    assert out.shape == (0, 64 * 24 + 64 * 9 + OW)
    L = ops.frame_layout('nv12', OH, OW, dict(pitch=64), 4096)
    assert render.render_video(_video(), vd, out_size=(OW, OH), out_fmt='nv12', out_layout=L).shape == (0, 4096)
    assert render.render_video(_video(), vd, out_size=(OW, OH)).shape == (0, OH, OW, 3)      # without one: as ever


@pytest.mark.parametrize('fmt,lay,text', MISMATCHED)
def test_render_crops_refuses_before_any_device_work(fmt, lay, text):
    eng = ops.Engine.__new__(ops.Engine)                        # no handle, no device: nothing below may need one
    frames = np.zeros((4, H, W, 3), np.uint8)                   # (not even a tensor: the layout's refusal comes first)
    boxes = np.array([[2, 4, 2 + OW, 4 + OH]] * 4, np.int32)
    with pytest.raises(ValueError) as e:
        eng.render_crops(frames, boxes, out_fmt=fmt, out_layout=lay)
    assert text in str(e.value)
    with pytest.raises(ValueError) as e:
        eng.render_crops(frames, np.array([[2, 4, 26, 20]] * 4, np.int32), out_hw=(OH, OW), out_fmt=fmt, out_layout=lay, interp='lanczos')
    assert text in str(e.value)
    with pytest.raises(TypeError) as e:                         # the engine's door takes the checked object, as layout= does
        eng.render_crops(frames, boxes, out_layout=dict(pitch=96))
    assert 'out_layout must be an ops.FrameLayout' in str(e.value)


def test_the_raw_writer_refuses_a_layout(tmp_path):
    path = str(tmp_path / 'out.raw')
    with pytest.raises(ValueError) as e:
        ingest.write_frames_raw(path, 25.0, (OW, OH), pix_fmt='nv12', layout=ops.frame_layout('nv12', OH, OW, dict(pitch=64)))
    assert 'packed' in str(e.value) and not os.path.exists(path)
    w = ingest.write_frames_raw(path, 25.0, (OW, OH), pix_fmt='nv12', layout=None)            # None: the writer it always was
    w.write(np.zeros((OH * 3 // 2, OW), np.uint8))
    w.release()
    assert os.path.getsize(path) == OH * OW * 3 // 2


@pytest.fixture
def writer_calls(monkeypatch):
    """A recording writer in smartVidCrop's hand-off; restored afterwards."""
    calls = []

    class Writer:
        def __init__(self):
            self.frames = []

        def write(self, f):
            self.frames.append(np.array(f))

        def release(self):
            pass

    def opened(path, fr, size, **kw):
        calls.append((path, size, kw, Writer()))
        return calls[-1][3]
    monkeypatch.setattr(S, '_video_writer', opened)
    return calls


@pytest.mark.parametrize('fmt,lay,text', BROKEN + MISMATCHED)
def test_smart_vid_crop_refuses_before_any_work_and_before_a_writer_is_opened(fmt, lay, text, writer_calls, monkeypatch):
    monkeypatch.setattr(S, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    with pytest.raises(ValueError) as e:
        S.smart_vid_crop(_video(), final_vid_fn='out.raw', out_size=(OW, OH), out_pix_fmt=fmt, out_layout=lay)
    assert text in str(e.value) and not writer_calls


def test_the_pickle_mode_has_no_layout(writer_calls, monkeypatch, tmp_path):
    monkeypatch.setattr(S, 'get_engine', lambda *a, **k: pytest.fail('an engine was asked for'))
    with pytest.raises(ValueError) as e:
        S.smart_vid_crop(str(tmp_path / 'video.pkl'), final_vid_fn='x', out_layout=dict(pitch=96))      # (the file is never opened)
    assert 'the pickle mode writes packed BGR crops' in str(e.value) and not writer_calls
    with pytest.raises(ValueError) as e:                        # a format mismatch is known without the size
        S.smart_vid_crop(_video(), final_vid_fn='x', out_pix_fmt='nv12', out_layout=ops.frame_layout('rgb24', OH, OW))
    assert 'out_layout is one of rgb24 frames' in str(e.value) and not writer_calls


def test_the_writer_receives_layout_only_when_one_was_given(writer_calls, monkeypatch):
    """smart_vid_crop with the analysis and the renderer replaced by stand-ins (no device): which keywords the writer is opened with
    and what render_video is handed -- the rule colour= follows."""
    vd = dict(_vd(), fr=25.0, fbb_w=OW, fbb_h=OH)
    monkeypatch.setattr(S, 'ingest_frames', lambda *a, **k: dict(vd))
    monkeypatch.setattr(S, 'after_ingest', lambda VD, CP, engine, verbose=False: (VD, {}))
    rendered = []

    def fake_render(video, VD, **kw):
        rendered.append(kw)
        kw['sink'](np.zeros((2, 7), np.uint8))
    monkeypatch.setattr(render, 'render_video', fake_render)
    eng = object()
    S.smart_vid_crop(_video(), final_vid_fn='a', engine=eng)
    S.smart_vid_crop(_video(), final_vid_fn='b', engine=eng, out_pix_fmt='nv12')
    S.smart_vid_crop(_video(), final_vid_fn='c', engine=eng, out_layout=dict(pitch=96))
    S.smart_vid_crop(_video(), final_vid_fn='d', engine=eng, out_pix_fmt='nv12', out_colour=('bt709', 'full'),
                     out_layout=dict(pitch=64, chroma_offset=64 * 24))
    L = ops.frame_layout('nv12', 40, 50, dict(pitch=64), 8192)
    S.smart_vid_crop(_video(), final_vid_fn='e', engine=eng, out_pix_fmt='nv12', out_size=(50, 40), out_layout=L)
    kws = [c[2] for c in writer_calls]
    assert [c[0] for c in writer_calls] == list('abcde')
    assert kws[0] == {} and kws[1] == dict(pix_fmt='nv12')      # the calls they always were
    assert kws[2] == dict(layout=ops.frame_layout('rgb24', OH, OW, dict(pitch=96)))
    assert kws[3] == dict(pix_fmt='nv12', colour=dict(matrix='bt709', range='full'),
                          layout=ops.frame_layout('nv12', OH, OW, dict(pitch=64, chroma_offset=64 * 24)))
    assert kws[4] == dict(pix_fmt='nv12', layout=L) and writer_calls[4][1] == (50, 40)
    assert [r['out_layout'] for r in rendered] == [None, None, kws[2]['layout'], kws[3]['layout'], L]
    assert all(len(c[3].frames) == 2 for c in writer_calls)
