"""The retargeted frames: every frame's crop window cut out of the full frame on the device (sc_renderer,
smartVidCrop.py:1801-1921; the crop itself is frame[by1:by2, bx1:bx2, :] at :1910), optionally resampled to a fixed
output size with cv2.resize(INTER_LINEAR) semantics (svc_render_crops_u8, include/svc.h).

    VD, res = S.smart_vid_crop(video, CP, save_vid=False)
    crops = render.render_video(video, VD)                            # uint8 [fc, fbb_h, fbb_w, 3] RGB
    render.render_video(video, VD, out_size=(1080, 1920), sink=enc)   # enc(chunk [m,1920,1080,3]) in frame order

The frames come from any container the ingest accepts, in either pixel format, packed or with a layout (frames.FrameSource
describes the kinds and reads them: a dict's pix_fmt='nv12' frames are converted inside the render kernels,
svc_render_crops_nv12, frames with a layout are staged as they are and read through it, svc_render_crops_layout; the crops
are those of the packed RGB pictures).  The crops are RGB / BGR -- unless out_fmt='nv12' asks for NV12 crops (uint8
[m, oh * 3 / 2, ow], what a hardware encoder takes: BT.601 limited range, fused into the render kernels,
svc_render_crops_u8_to_nv12 / _nv12_to_nv12; half the bytes to copy back).  They come back through pinned double buffers on
a second side stream, so that the sink consumes chunk c while the device renders chunk c + 1.  out_layout= renders them into an
encoder's layout instead (svc_render_crops_to_layout): chunks uint8 [m, frame_stride], picture bytes in place, 0 elsewhere."""
import numpy as np

_MAX_CHUNK = 32
_RING_BYTES = 96 << 20         # one output slot (device and pinned, two of each per engine): at most this many bytes


def check_boxes(bbs, fc, h, w):
    """bbs [fc,4] (x1,y1,x2,y2) -> (bw, bh); ValueError unless every window has the same size and lies inside the frame."""
    b = np.asarray(bbs, np.int64)
    if b.ndim != 2 or b.shape != (fc, 4):
        raise ValueError('expected %d boxes [x1,y1,x2,y2], got shape %s' % (fc, b.shape))
    bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    if fc and (np.any(bw != bw[0]) or np.any(bh != bh[0])):
        raise ValueError('crop windows differ in size (%s x %s ... %s x %s)' % (bw.min(), bh.min(), bw.max(), bh.max()))
    if fc and (bw[0] < 1 or bh[0] < 1):
        raise ValueError('empty crop window %d x %d' % (bw[0], bh[0]))
    bad = np.flatnonzero((b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] > w) | (b[:, 3] > h))
    if bad.size:
        raise ValueError('crop window of frame %d %s lies outside the %d x %d frame' % (bad[0], b[bad[0]].tolist(), w, h))
    return (int(bw[0]), int(bh[0])) if fc else (0, 0)


def render_video(video, VD, engine=None, out_size=None, bgr=False, sink=None, chunk=32, pix_fmt=None, out_fmt='rgb24', layout=None,
                 interp='linear', colour=None, out_colour=None, out_layout=None, subpixel=False):
    """Render VD['fc'] frames of `video` (the ingest_pickle dict, or its 'frames' container) at VD['bbs_np'].
    pix_fmt: the frames' format when `video` is a bare container (a dict brings its own 'pix_fmt'; default 'rgb24'); an
    unknown format, an NV12 picture of odd size or a container of another shape raise ValueError before any device work.
    out_size: (w, h) of the output frames (None = the window size, an exact copy); bgr: R and B swapped (the reference's
    pickle mode); sink: called with every chunk uint8 [m, oh, ow, 3] (m <= chunk) in frame order -- a view of a pinned
    buffer that is refilled after the call returns, so copy what you keep.  -> numpy uint8 [fc, oh, ow, 3] without a sink,
    else None.  Boxes of unequal size or outside the frame raise ValueError before any device work.
    out_fmt='nv12': chunks and the returned array are NV12 frames uint8 [m, oh * 3 / 2, ow] (include/svc.h states the formula);
    an odd output size (pass an even out_size), bgr with it, or an unknown format raise ValueError before any device work.
    layout: the ops.FrameLayout of a bare container of uint8 [n, frame_stride] frames (a dict brings its own 'layout').
    interp: the filter an out_size is resampled with, one of ops.INTERPS: 'linear' (cv2.resize INTER_LINEAR) or 'lanczos'
    (PIL.Image.resize LANCZOS on the cropped window, bit for bit); another value raises ValueError before any device work.
    colour: the matrix and range of a bare container of nv12 frames (a dict brings its own 'colour'; ops.frame_colour states the
    spellings).  out_colour: the colour an nv12 output is encoded with; None means the source's (BT.601 limited for an rgb24
    source).  With out_fmt='rgb24' a given out_colour raises ValueError, as does an unknown matrix or range.
    out_layout: where the bytes of every output frame lie, as an encoder's surfaces want them -- dict(pitch=, chroma_offset=,
    chroma_pitch=) (frames their extent apart) or an ops.FrameLayout of the out_fmt picture of the final size; resolved once,
    against the final (oh, ow), and a broken rule or another format or size raises ValueError before any device work.  Chunks
    and the returned array are then uint8 [m, frame_stride]: the picture bytes are those of the call without it, every other
    byte is 0 (svc_render_crops_to_layout writes the picture rows and nothing else, into slots that were allocated zeroed).
    subpixel: render the windows at VD['bbs_q8'] -- their origins in 1/256 pixel, as sc_compute_bb keeps them from the smoothed
    centres before the truncation -- instead of at the whole pixels of VD['bbs_np'], so that a crop delivered at an out_size follows
    the smoothed pan without steps (svc_render_windows_q8; include/svc.h states the arithmetic; the window size stays that of
    VD['bbs_np']).  Every other option as without it; without an out_size the window is shifted by its fraction.  With
    interp='lanczos' (the phase is defined on the INTER_LINEAR taps), or a VD without 'bbs_q8': ValueError before any device work."""
    from .frames import FrameSource
    from .ops import check_interp, frame_colour
    check_interp(interp)
    if subpixel and interp != 'linear':
        raise ValueError("subpixel=True renders with interp='linear' (the phase shifts the INTER_LINEAR taps), not %r" % (interp,))
    if subpixel and VD.get('bbs_q8') is None:
        raise ValueError("subpixel=True needs VD['bbs_q8'] (sc_compute_bb sets it); this VD has none")
    src = FrameSource.of(video, pix_fmt, layout, colour).whole()       # (resolved and checked once)
    if out_colour is not None:
        out_colour = frame_colour(out_colour)
        if out_fmt == 'rgb24':
            raise ValueError("out_colour=%r describes an nv12 output; out_fmt is 'rgb24'" % (out_colour,))
    elif out_fmt == 'nv12':
        out_colour = src.colour                                 # (None for an rgb24 source: BT.601 limited)
    fc = int(VD['fc'])
    if src.n < fc:
        raise ValueError('the container holds %d frames, the video has %d' % (src.n, fc))
    bw, bh = check_boxes(VD['bbs_np'][:fc] if fc else np.zeros((0, 4)), fc, src.h, src.w)
    ow, oh = (bw, bh) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if oh < 1 or ow < 1:
        raise ValueError('output size %s' % (out_size,))
    from .ops import out_frame_shape, out_layout_of
    shape = out_frame_shape(out_fmt, oh, ow, bgr)
    out_layout = out_layout_of(out_layout, out_fmt, oh, ow)
    if out_layout is not None:
        shape = (out_layout.frame_stride,)
    if subpixel:
        q8 = np.asarray(VD['bbs_q8'])[:fc]
        if q8.shape != (fc, 2) or q8.dtype.kind not in 'iu':
            raise ValueError("VD['bbs_q8'] holds integer origins [fc, 2] (x, y in 1/256 pixel), not %s %s" % (q8.dtype, q8.shape))
        q8 = np.clip(q8, -2 ** 31, 2 ** 31 - 1).astype(np.int32)          # (the kernel clamps into the frame)
    chunk = max(1, min(int(chunk), _MAX_CHUNK, _RING_BYTES // int(np.prod(shape))))       # (the real bytes per frame)
    result = None
    if sink is None:
        result = np.empty((fc,) + shape, np.uint8)

        def sink(c, _pos=[0]):
            result[_pos[0]:_pos[0] + c.shape[0]] = c
            _pos[0] += c.shape[0]
    if fc == 0:
        return result
    import torch
    from . import smartVidCrop as S
    engine = engine or S.get_engine()
    dev = engine.device
    boxes = torch.from_numpy(np.ascontiguousarray(q8 if subpixel else VD['bbs_np'][:fc], np.int32)).to(dev)      # subpixel: the origins
    out = _OutRing(engine, chunk, oh, ow, sink, out_fmt, src.pix_fmt, src.layout, interp, src.colour, out_colour, out_layout, subpixel)
    src.chunks(engine, fc, chunk, lambda staged, s: out.push(staged, boxes[s:s + staged.shape[0]], bw, bh, bgr))
    out.flush()
    return result


class _OutRing:
    """Two device output slots and two pinned host slots: chunk c is rendered on the caller's stream into device slot c & 1,
    copied D2H on a side stream into pinned slot c & 1, and handed to the sink once the copy of chunk c + 1 is enqueued."""

    def __init__(self, engine, cap, oh, ow, sink, out_fmt='rgb24', pix_fmt='rgb24', layout=None, interp='linear', colour=None, out_colour=None,
                 out_layout=None, subpixel=False):
        import torch
        from .ops import frame_shape
        self.engine, self.sink, self.dev, self.out_fmt = engine, sink, engine.device, out_fmt
        self.pix_fmt, self.layout = pix_fmt, layout             # of the frames that will be pushed
        self.interp = interp
        self.colour, self.out_colour = colour, out_colour       # of nv12 frames pushed / of an nv12 output (None: BT.601 limited)
        self.out_layout = out_layout                            # of the output frames (None: packed)
        self.subpixel = subpixel                                # push() is handed origins [m, 2] in 1/256 pixel, not boxes
        key = (cap, oh, ow, out_fmt) if out_layout is None else (cap, oh, ow, out_fmt, out_layout.key())
        # slots shaped (and keyed) by the output format -- and by the output layout: [cap, frame_stride], allocated zeroed, and
        # the kernels write picture bytes only, so what is delivered is 0 outside the picture for as long as the slots live
        shape = (cap,) + (frame_shape(out_fmt, oh, ow) if out_layout is None else (out_layout.frame_stride,))
        make = torch.empty if out_layout is None else torch.zeros
        ring = engine.__dict__.get('_render_ring')
        if ring is None or ring['key'] != key:
            ring = engine._render_ring = dict(
                key=key, dev=[make(shape, dtype=torch.uint8, device=self.dev) for _ in range(2)],
                host=[make(shape, dtype=torch.uint8).pin_memory() for _ in range(2)],
                stream=torch.cuda.Stream(device=self.dev))
        self.ring = ring
        self.rendered = [torch.cuda.Event(), torch.cuda.Event()]
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]
        self.used = [False, False]
        self.c = 0
        self.pending = None                 # (slot, frames) of the chunk whose D2H is in flight

    def push(self, staged, boxes, bw, bh, bgr):
        m = int(staged.shape[0])
        cap = self.ring['key'][0]
        for s in range(0, m, cap):          # (a host feed stages at most 32 frames, the ring holds `chunk`)
            self._one(staged[s:s + cap], boxes[s:s + cap], bw, bh, bgr)

    def _one(self, staged, boxes, bw, bh, bgr):
        import torch
        m = int(staged.shape[0])
        slot = self.c & 1
        compute = torch.cuda.current_stream(self.dev)
        side = self.ring['stream']
        if self.used[slot]:
            compute.wait_event(self.copied[slot])           # the device slot's previous D2H has read it
        dst = self.ring['dev'][slot][:m]
        if self.subpixel:
            self.engine.render_windows(staged, boxes, (bw, bh), (int(self.ring['key'][1]), int(self.ring['key'][2])), bgr, dst, self.pix_fmt,
                                       self.out_fmt, self.layout, self.colour, self.out_colour, self.out_layout)
        else:
            self.engine._render(staged, boxes, bw, bh, dst, bgr, self.pix_fmt, self.out_fmt, self.layout, self.interp, self.colour, self.out_colour,
                                self.out_layout)
        self.rendered[slot].record(compute)
        with torch.cuda.stream(side):
            side.wait_event(self.rendered[slot])
            self.ring['host'][slot][:m].copy_(dst, non_blocking=True)
            self.copied[slot].record(side)
        self.used[slot] = True
        prev, self.pending = self.pending, (slot, m)
        if prev is not None:
            self._deliver(prev)
        self.c += 1

    def _deliver(self, what):
        slot, m = what
        self.copied[slot].synchronize()
        self.sink(self.ring['host'][slot][:m].numpy())

    def flush(self):
        if self.pending is not None:
            self._deliver(self.pending)
            self.pending = None
