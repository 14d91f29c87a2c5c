"""Rendering without a GPU: argument checks of svc_render_crops_u8, box validation of render.render_video before any
device work, the Pillow frame writer, and the parts of smart_vid_crop's save_vid door that stay unsupported."""
import ctypes

import numpy as np
import pytest

from retargetvid_amd import _lib, ingest, render, smartVidCrop as S


def test_render_entry_checks_its_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(16)                   # never dereferenced: every call below fails validation first
    ok = dict(h=fake, frames=fake, n=2, height=360, width=640, boxes=fake, bw=120, bh=360, out=fake, oh=360, ow=120, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.svc_render_crops_u8(a['h'], a['frames'], a['n'], a['height'], a['width'], a['boxes'], a['bw'], a['bh'],
                                       a['out'], a['oh'], a['ow'], a['flags'], None)
    assert call(h=None) == -1 and b'svc_render_crops_u8' in lib.svc_last_error()
    for bad in (dict(n=-1), dict(height=0), dict(width=0), dict(bw=0), dict(bh=0), dict(oh=0), dict(ow=0),
                dict(bw=641), dict(bh=361), dict(flags=2), dict(flags=-1), dict(frames=None), dict(boxes=None), dict(out=None),
                dict(oh=100, ow=30000)):                 # a resampled output row beyond the LDS budget
        assert call(**bad) == -1, bad


def _vd(boxes):
    return dict(fc=len(boxes), bbs_np=np.asarray(boxes, np.int64))


def test_render_video_rejects_bad_boxes_before_device_work():
    frames = np.zeros((3, 36, 64, 3), np.uint8)
    for boxes in ([[0, 0, 10, 36], [1, 0, 11, 36], [2, 0, 13, 36]],        # unequal widths
                  [[0, 0, 10, 36], [1, 1, 11, 36], [2, 0, 12, 36]],        # unequal heights
                  [[-1, 0, 9, 36], [1, 0, 11, 36], [2, 0, 12, 36]],        # left of the frame
                  [[0, 0, 10, 36], [55, 0, 65, 36], [2, 0, 12, 36]],       # right of the frame
                  [[0, 1, 10, 37], [0, 1, 10, 37], [0, 1, 10, 37]],        # below the frame
                  [[0, 0, 0, 36], [0, 0, 0, 36], [0, 0, 0, 36]],           # empty
                  [[0, 0, 10, 36], [1, 0, 11, 36]]):                      # fewer boxes than frames
        VD = _vd(boxes)
        VD['fc'] = 3
        with pytest.raises(ValueError):
            render.render_video(frames, VD, engine=None)           # engine None: a device engine would be built after the checks
    with pytest.raises(ValueError):                                 # a container with fewer frames than the video
        render.render_video(frames[:2], _vd([[0, 0, 10, 36]] * 3), engine=None)
    assert render.check_boxes(np.array([[0, 0, 64, 36], [0, 0, 64, 36]]), 2, 36, 64) == (64, 36)


def test_pillow_writer_round_trip(tmp_path):
    frames = np.random.RandomState(0).randint(0, 256, (5, 19, 23, 3)).astype(np.uint8)
    out = str(tmp_path / 'clip')
    w = ingest.write_frames_pillow(out, 25.0, (23, 19))
    for f in frames:
        w.write(f)
    w.release()
    back = ingest.read_frames_pillow(out, fr=25.0)
    assert np.array_equal(back['frames'], frames) and back['fr'] == 25.0
    with pytest.raises(ValueError):
        ingest.write_frames_pillow(str(tmp_path / 'other'), 25.0, (23, 19)).write(frames[0][:, :20])


def test_unsupported_render_outputs_raise():
    video = dict(fr=30.0, frame_count=3, w=64, h=36, frames=np.zeros((3, 36, 64, 3), np.uint8), trans_inds=[0, 3])
    with pytest.raises(NotImplementedError, match='demo'):
        S.smart_vid_crop(video, demo_fn='demo')
    with pytest.raises(NotImplementedError, match='copy_sound'):
        S.smart_vid_crop(video, final_vid_fn='out', copy_sound=True)
    S.set_video_writer(None)
    with pytest.raises(NotImplementedError, match='set_video_writer'):
        S.smart_vid_crop(video, final_vid_fn='out')
