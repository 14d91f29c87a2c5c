"""Optional decode hand-off in front of the path.

The saliency-to-crop path starts at decoded RGB frames (the reference's ``ingest_pickle`` door,
smartVidCrop.py:560-836).  Decoding and TransNetV1 shot detection stay on the host and outside
this package; this module only adapts a decoder to that door:

    from retargetvid_amd import ingest, smartVidCrop as S
    S.set_video_reader(lambda path, CP: ingest.read_video_cv2(path, shot_detector=my_transnet))
    VD, res = S.smart_vid_crop('clip.mp4', CP, save_vid=False)

``read_video_cv2`` needs OpenCV (``cv2``), which is not part of this image (it has never run here); ``shot_detector`` is
any callable ``frames[n,h,w,3] u8 RGB -> iterable of transition frame indices`` (the reference runs TransNetV1 at 27x48,
transnetv1_handler.py:91-130, and thresholds its output with ``t_cut``); without one the video is a single shot.

``read_frames_pillow`` is the decoder that DOES run in this image (Pillow is installed; tests/test_host_logic.py and
tests/test_gpu_pipeline.py execute it): a directory of frame images (a video extracted to PNG / JPEG files, sorted by name) or
one multi-frame image file (GIF, APNG, WebP, TIFF).  ``shots=None`` leaves ``trans_inds`` out of the dict, so that
``smart_vid_crop(path, CP, shot_net=net)`` takes the reference's video path (TransNet V1 on the device decides the shots):

    S.set_video_reader(lambda path, CP: ingest.read_frames_pillow(path, fr=25.0, shots=None))
    VD, res = S.smart_vid_crop('frames_of_clip_017/', CP, save_vid=False, shot_net=net)

The way out mirrors the way in: ``write_frames_pillow`` is a writer for smartVidCrop.set_video_writer that stores the
rendered frames as a lossless PNG frame folder, which ``read_frames_pillow`` reads back bit for bit:

    S.set_video_writer(ingest.write_frames_pillow)
    VD, res = S.smart_vid_crop('frames_of_clip_017/', CP, final_vid_fn='clip_017_9x16/')

``write_frames_raw`` is the writer for an encoder: one file of raw frames, RGB or -- rendered as such on the device -- NV12,
which ``ffmpeg -f rawvideo -pix_fmt nv12 -s 1080x1920 -r 25 -i clip_017.nv12 ...`` reads:

    S.set_video_writer(ingest.write_frames_raw)
    VD, res = S.smart_vid_crop(video, CP, final_vid_fn='clip_017.nv12', out_size=(1080, 1920), out_pix_fmt='nv12')
"""
import os

import numpy as np


def video_dict(frames, fr, trans_inds=None, frame_count=None, shots='given'):
    """The ingest_pickle dict (smartVidCrop.py:568-573) for decoded RGB frames [n,h,w,3] u8.  shots=None: no ``trans_inds``
    key (the entry point then runs shot detection itself: smart_vid_crop(..., shot_net=))."""
    n, h, w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    fc = int(frame_count) if frame_count is not None else n
    out = dict(fr=float(fr), frame_count=fc, w=w, h=h, frames=frames)
    if shots is not None:
        ti = sorted(set(int(t) for t in (trans_inds or []) if 0 < int(t) < n))
        out['trans_inds'] = [0] + ti + [n]
    return out


_IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff', '.webp', '.ppm')


def read_frames_pillow(path, fr=None, shot_detector=None, max_frames=None, shots='given'):
    """Decode with Pillow into the ingest_pickle dict: ``path`` = a directory of frame images (sorted by file name; all of one
    size) or one multi-frame image file (GIF / APNG / WebP / TIFF).  Frames are converted to RGB like the reference's
    cv2.cvtColor(frame, COLOR_BGR2RGB) (smartVidCrop.py:330-331).  ``fr``: frames per second; None = the file's own frame
    duration where it has one (GIF / APNG / WebP ``duration`` in ms), else 25.0.  ``shot_detector`` / ``shots`` as in video_dict."""
    from PIL import Image
    out, rate = [], fr
    if os.path.isdir(path):
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(_IMAGE_EXT))
        if not names:
            raise IOError('no frame images in %r' % (path,))
        for f in names[:max_frames]:
            with Image.open(os.path.join(path, f)) as im:
                out.append(np.asarray(im.convert('RGB'), np.uint8))
    else:
        with Image.open(path) as im:
            n = int(getattr(im, 'n_frames', 1))
            if rate is None and im.info.get('duration'):
                rate = 1000.0 / float(im.info['duration'])
            for i in range(n if max_frames is None else min(n, max_frames)):
                im.seek(i)
                out.append(np.asarray(im.convert('RGB'), np.uint8))
    if any(f.shape != out[0].shape for f in out):
        raise IOError('frames of %r differ in size' % (path,))
    frames = np.ascontiguousarray(np.stack(out))
    trans = list(shot_detector(frames)) if shot_detector is not None else []
    return video_dict(frames, 25.0 if rate is None else rate, trans, shots=shots)


class _PillowFrameWriter:
    def __init__(self, path, fr, size):
        os.makedirs(path, exist_ok=True)
        self.path, self.fr, self.size, self.n = path, float(fr), (int(size[0]), int(size[1])), 0

    def write(self, frame_rgb_u8):
        from PIL import Image
        f = np.ascontiguousarray(frame_rgb_u8, np.uint8)
        if f.shape != (self.size[1], self.size[0], 3):
            raise ValueError('frame of shape %s, the writer was opened for %d x %d' % (f.shape, self.size[0], self.size[1]))
        Image.fromarray(f, 'RGB').save(os.path.join(self.path, '%06d.png' % self.n), compress_level=1)
        self.n += 1

    def release(self):
        pass


def write_frames_pillow(path, fr, size, pix_fmt='rgb24'):
    """The encode side of read_frames_pillow, in the shape of cv2.VideoWriter (smartVidCrop.set_video_writer):
    ``write(frame)`` stores RGB [h,w,3] u8 frames of ``size`` = (w, h) as ``path/000000.png``, ``000001.png``, ... (lossless;
    the directory is created), ``release()`` ends it.  ``fr`` is accepted for the writer signature; a PNG folder keeps no
    frame rate (read_frames_pillow(path, fr=...) gives it back).  A PNG holds RGB: any other ``pix_fmt`` (smart_vid_crop's
    out_pix_fmt='nv12') is refused with ValueError; write_frames_raw takes NV12."""
    if pix_fmt != 'rgb24':
        raise ValueError('write_frames_pillow stores RGB frames as PNG files, not pix_fmt=%r: use write_frames_raw' % (pix_fmt,))
    return _PillowFrameWriter(path, fr, size)


class _RawFrameWriter:
    def __init__(self, path, fr, size, pix_fmt):
        w, h = int(size[0]), int(size[1])
        if pix_fmt == 'rgb24':
            self.shape = (h, w, 3)
        elif pix_fmt == 'nv12':
            if w < 2 or h < 2 or w % 2 or h % 2:
                raise ValueError('an nv12 picture has even width and height (>= 2), not %d x %d' % (w, h))
            self.shape = (h * 3 // 2, w)
        else:
            raise ValueError('unknown pix_fmt %r (rgb24 or nv12)' % (pix_fmt,))
        self.path, self.fr, self.size, self.pix_fmt, self.n = path, float(fr), (w, h), pix_fmt, 0
        self.fp = open(path, 'wb')

    def write(self, frame_u8):
        f = np.ascontiguousarray(frame_u8, np.uint8)
        if f.shape != self.shape:
            raise ValueError('frame of shape %s, the writer was opened for %s frames of %d x %d' % ((f.shape, self.pix_fmt) + self.size))
        self.fp.write(f.data)
        self.n += 1

    def release(self):
        self.fp.close()


def write_frames_raw(path, fr, size, pix_fmt='rgb24', colour=None, layout=None):
    """A writer for smartVidCrop.set_video_writer that appends every frame's bytes to the one file ``path``: a raw stream
    as ``ffmpeg -f rawvideo -pix_fmt <pix_fmt> -s <w>x<h> -r <fr>`` reads it.  ``pix_fmt``: 'rgb24' (frames [h,w,3] u8) or
    'nv12' (frames [h*3/2,w] u8, w and h even: smart_vid_crop(..., out_pix_fmt='nv12')); ``size`` = (w, h).  A raw file keeps
    neither size nor rate nor colour: ``fr``, and the ``colour=dict(matrix=, range=)`` that smart_vid_crop hands over for an NV12
    output that is not BT.601 limited, are accepted for the writer signature and ignored.  ``layout``: what
    smart_vid_crop(out_layout=...) hands its writer; a raw file is packed, so anything but None is refused with ValueError (before
    the file is created).  Needs nothing beyond numpy."""
    if layout is not None:
        raise ValueError('write_frames_raw writes packed frames: a raw file has no pitch (layout=%r); render without out_layout' % (layout,))
    return _RawFrameWriter(path, fr, size, pix_fmt)


def read_video_cv2(path, shot_detector=None, max_frames=None):
    """Decode a file with OpenCV (BGR -> RGB, like smartVidCrop.py:330-331) into the ingest_pickle dict."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError('read_video_cv2 needs OpenCV (cv2); install it or pass your own reader to '
                          'smartVidCrop.set_video_reader()') from e
    cap = cv2.VideoCapture(path)
    if not cap.isOpened():
        raise IOError('cannot open video %r' % (path,))
    fr = cap.get(cv2.CAP_PROP_FPS)
    frame_count = int(cap.get(cv2.CAP_PROP_FRAME_COUNT))
    out = []
    while max_frames is None or len(out) < max_frames:
        ok, bgr = cap.read()
        if not ok:
            break
        out.append(np.ascontiguousarray(bgr[:, :, ::-1]))
    cap.release()
    if not out:
        raise IOError('no frames decoded from %r' % (path,))
    frames = np.stack(out)
    trans = list(shot_detector(frames)) if shot_detector is not None else []
    return video_dict(frames, fr, trans, frame_count=max(frame_count, len(out)))
