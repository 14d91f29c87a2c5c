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
        if self.subpixel:
            self.put(int(staged.shape[0]), lambda dst: self.engine.render_windows(
                staged, boxes, (bw, bh), (int(self.ring['key'][1]), int(self.ring['key'][2])), bgr, dst, self.pix_fmt, self.out_fmt, self.layout,
                self.colour, self.out_colour, self.out_layout))
        else:
            self.put(int(staged.shape[0]), lambda dst: self.engine._render(
                staged, boxes, bw, bh, dst, bgr, self.pix_fmt, self.out_fmt, self.layout, self.interp, self.colour, self.out_colour, self.out_layout))

    def put(self, m, fill):
        """One chunk of m <= cap frames: fill(dst) enqueues on the current stream whatever writes them into dst, the device slot's
        first m frames; the ring copies them back and delivers them in order.  (What push() does per chunk; render_demo's door.)"""
        import torch
        slot = self.c & 1
        compute = torch.cuda.current_stream(self.dev)
        side = self.ring['stream']
        if self.used[slot]:
            compute.wait_event(self.copied[slot])           # the device slot's previous D2H has read it
        dst = self.ring['dev'][slot][:m]
        fill(dst)
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


# --------------------------------------------------------------------------------------------------------------------------
# The five-panel demo video (sc_renderer, smartVidCrop.py:1924-2126): frame | raw saliency | filtered map with the centre's
# trail, the jump score and the cut labels | overlay | frame with the final window.  The host states WHAT is drawn, per frame, as
# a list of integer marks (demo_marks); the device composes the panels and draws the marks (ops.demo_frames:
# svc_demo_frames_u8, include/svc.h states the pixel rules).  The marks are this package's own rasterising rules, not
# OpenCV's: no anti-aliased circles and lines, and the labels are Pillow's default font, not the Hershey glyphs.
# --------------------------------------------------------------------------------------------------------------------------
DEMO_FONT_POS, DEMO_FONT_POS2, DEMO_FONT_POS3, DEMO_FONT_POS4 = (2, 15), (2, 30), (2, 45), (2, 60)      # smartVidCrop.py:1858-1862
DEMO_TITLES = ((1, 'saliency'), (2, 'filtered'), (3, 'overlayed'), (4, 'final'))                        # (panel, title), :2086-2117
DEMO_STRINGS = tuple(t for _, t in DEMO_TITLES) + ('jump:', 'jump', 'orig. cut') + tuple('0123456789')
_DEMO_ATLAS = None


def demo_atlas():
    """The label sprites, built once per process with Pillow's default font -> (atlas uint8 [bytes], {string: (offset, w, h)}) for
    every string of DEMO_STRINGS.  A sprite is w x h coverages (0 .. 255), row-major at atlas[offset:]: the string drawn at (2, 1)
    in a box of its advance width + 4 and the font's line height + 2 (a margin that keeps an empty pixel all around the glyphs'
    anti-aliased edges, for the outline), so every sprite has the same height and baseline and strings are composed by placing
    them w - 4 apart ('jump:%d' from 'jump:' and the digits).  Directly behind it, at offset + w * h
    and of the same size, lies its 3 x 3 dilation (the maximum over the neighbourhood): the black outline drawn under the label."""
    global _DEMO_ATLAS
    if _DEMO_ATLAS is None:
        from PIL import Image, ImageDraw, ImageFont
        font = ImageFont.load_default()
        box = font.getbbox('Mgjy|0123456789')
        line = int(box[3]) + 1
        parts, where, pos = [], {}, 0
        for s in DEMO_STRINGS:
            w, h = int(np.ceil(font.getlength(s))) + 4, line + 2
            img = Image.new('L', (w, h), 0)
            ImageDraw.Draw(img).text((2, 1), s, fill=255, font=font)
            a = np.asarray(img, np.uint8)
            pad = np.pad(a, 1)
            d = np.max([pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0).astype(np.uint8)
            where[s] = (pos, w, h)
            parts += [a.reshape(-1), d.reshape(-1)]
            pos += 2 * w * h
        _DEMO_ATLAS = (np.ascontiguousarray(np.concatenate(parts)), where)
    return _DEMO_ATLAS


def _demo_label(rows, where, panel, pos, strings):
    """The label made of `strings` side by side, its bottom-left corner at pos (cv2.putText's org): every string's dilated
    sprite in black, then every string in white."""
    from ._lib import MARK_TEXT
    for dilated, colour in ((1, 0), (0, 0xffffff)):
        x = int(pos[0]) - 2
        for s in strings:
            off, w, h = where[s]
            rows.append((MARK_TEXT | panel << 8, x, int(pos[1]) - (h - 2), 0, 0, off + dilated * w * h, w | h << 16, colour))
            x += w - 4


def demo_marks(VD, CP):
    """What sc_renderer draws on the demo frames (smartVidCrop.py:1941-2117), in its draw order, as the marks ops.demo_frames
    takes -> (marks int32 [k, 8], first int32 [fc + 1], map_of int32 [fc]): the marks of frame i are rows first[i] .. first[i + 1],
    its maps are those of index map_of[i] = VD['inds_to_orig'][i].  int() truncation everywhere, as there.  With m = map_of[i],
    T = past_steps - j, past_steps = int(fr / 5) and the colour level max(0, 255 - 20 j - 20) of trail step j = 1 .. past_steps - 1:
      panel 2   where (dxnf, dynf)[m] != (dx, dy)[m]: the non-fixed centre in red -- a disc of radius 5, trail discs of radius
                2 + T // 2 at m - j (when i - j >= 0), trail lines of thickness T from m - j to m - j - 1 (when i - j > 0); then the
                centre (dx, dy) the same in green; 'jump:%d' % jumps[m] at DEMO_FONT_POS2; 'jump' at DEMO_FONT_POS3 while its counter
                runs (set to fade_len = fr by a jump below CP['foces_stab_t'], one less per frame) and 'orig. cut' at DEMO_FONT_POS4
                likewise (set by a frame index found in VD['segm_backup'])
      panel 3   a green disc of radius 3 at the centre
      panel 4   a green disc of radius 3 at (int(dxs * scale_w), int(dys * scale_h)) and the rectangle (int(bx1 * scale_w) + 1,
                int(by1 * scale_h) + 1, int(bx2 * scale_w) - 1, int(by2 * scale_h) - 1)
      panels 1 - 4   their titles at DEMO_FONT_POS
    Every label is its black 3 x 3-dilated sprite, then the white one (demo_atlas).  The marks are opaque: the reference's fading
    alpha lands in a channel that COLOR_BGRA2BGR drops (:2054).  A frame takes at most 64 marks (svc_demo_frames_u8): at fr >= 45
    the two trails alone reach that, and what comes later in the order -- the titles last -- is not drawn.
    Deviations from the reference, on purpose:
      * where it indexes before the start of a list (m - j < 0, m - j - 1 < 0: Python wraps around to the video's END), nothing is drawn;
      * 'jump' is drawn at DEMO_FONT_POS3 in both colours (the reference puts its white copy at DEMO_FONT_POS6, 45 rows lower)."""
    from ._lib import MARK_DISC, MARK_LINE, MARK_RECT, MARK_WORDS
    _, where = demo_atlas()
    fr, fc = VD['fr'], int(VD['fc'])
    m = [int(v) for v in VD['inds_to_orig'][:fc]]
    scale_h, scale_w = float(VD['h_process']) / float(VD['h_orig']), float(VD['w_process']) / float(VD['w_orig'])
    fade_len, past_steps = fr, int(fr / 5.0)
    cuts = set(int(v) for v in np.asarray(VD['segm_backup']).reshape(-1))
    bbs = VD['bbs_np'] if 'bbs_np' in VD else VD['bbs']
    green = 255 << 8
    fade_jump = fade_cut = 0
    rows, first = [], [0]

    def trail(xs, ys, i, mi, shift):
        rows.append((MARK_DISC | 2 << 8, int(xs[mi]), int(ys[mi]), 0, 0, 5, 0, 255 << shift))
        for j in range(1, past_steps):
            if i - j >= 0 and mi - j >= 0:
                rows.append((MARK_DISC | 2 << 8, int(xs[mi - j]), int(ys[mi - j]), 0, 0, 2 + (past_steps - j) // 2, 0, max(0, 255 - 20 * j - 20) << shift))
        for j in range(1, past_steps):
            if i - j > 0 and mi - j - 1 >= 0:
                rows.append((MARK_LINE | 2 << 8, int(xs[mi - j]), int(ys[mi - j]), int(xs[mi - j - 1]), int(ys[mi - j - 1]), past_steps - j, 0,
                             max(0, 255 - 20 * j - 20) << shift))
    for i in range(fc):
        mi = m[i]
        if VD['dxnf'][mi] != VD['dx'][mi] or VD['dynf'][mi] != VD['dy'][mi]:
            trail(VD['dxnf'], VD['dynf'], i, mi, 0)
        trail(VD['dx'], VD['dy'], i, mi, 8)
        _demo_label(rows, where, 2, DEMO_FONT_POS2, ['jump:'] + list('%d' % VD['jumps'][mi]))
        if VD['jumps'][mi] < CP['foces_stab_t']:
            fade_jump = fade_len
        if fade_jump > 0:
            _demo_label(rows, where, 2, DEMO_FONT_POS3, ['jump'])
            fade_jump -= 1
        if i in cuts:
            fade_cut = fade_len
        if fade_cut > 0:
            _demo_label(rows, where, 2, DEMO_FONT_POS4, ['orig. cut'])
            fade_cut -= 1
        rows.append((MARK_DISC | 3 << 8, int(VD['dx'][mi]), int(VD['dy'][mi]), 0, 0, 3, 0, green))
        bx1, by1, bx2, by2 = (int(v) for v in bbs[i])
        rows.append((MARK_DISC | 4 << 8, int(VD['dxs'][i] * scale_w), int(VD['dys'][i] * scale_h), 0, 0, 3, 0, green))
        rows.append((MARK_RECT | 4 << 8, int(bx1 * scale_w) + 1, int(by1 * scale_h) + 1, int(bx2 * scale_w) - 1, int(by2 * scale_h) - 1, 0, 0, green))
        for panel, title in DEMO_TITLES:
            _demo_label(rows, where, panel, DEMO_FONT_POS, [title])
        first.append(len(rows))
    marks = np.clip(np.asarray(rows, np.int64).reshape(-1, MARK_WORDS), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return marks, np.asarray(first, np.int32), np.asarray(m, np.int32)


def render_demo(video, VD, CP, engine=None, sink=None, chunk=32, bgr=False):
    """The demo frames of VD['fc'] frames of `video` (what render_video takes: any container, format, layout and colour) ->
    numpy uint8 [fc, h_process, 5 * w_process, 3] without a sink, else None: sink(chunk uint8 [m, h_process, 5 * w_process, 3]) is
    called in frame order with views of a pinned buffer, as render_video's.  Per chunk: the frames are staged as for render_video,
    brought to the process size by the ingest's own resize (engine.resize_frames: panel 0 is bit for bit the ingest's small frame),
    composed with VD['smaps_orig_dev'] (the raw maps), VD['smaps_dev'] (the filtered ones) and the marks of demo_marks(VD, CP) by one
    launch (ops.demo_frames), and copied back through the renderer's pinned double buffers.  bgr: (b, g, r) pixels.
    VD['smaps_orig_dev'] is kept by after_ingest(keep_raw=True) -- smart_vid_crop(demo_fn=) asks for it; a VD without it, or with
    maps of another shape than (h_process, w_process), raises ValueError before any device work."""
    from .frames import FrameSource
    if not dict.__contains__(VD, 'smaps_orig_dev') or VD['smaps_orig_dev'] is None:
        raise ValueError("render_demo needs the raw maps VD['smaps_orig_dev'] (after_ingest(keep_raw=True) keeps them; "
                         "the threshold overwrites VD['smaps_dev'] in place)")
    src = FrameSource.of(video).whole()
    fc, ph, pw = int(VD['fc']), int(VD['h_process']), int(VD['w_process'])
    if src.n < fc:
        raise ValueError('the container holds %d frames, the video has %d' % (src.n, fc))
    raw, filt = VD['smaps_orig_dev'], VD['smaps_dev']
    if tuple(raw.shape) != tuple(filt.shape) or tuple(filt.shape[1:]) != (ph, pw):
        raise ValueError('maps of shape %s / %s for a process size of %d x %d' % (tuple(raw.shape), tuple(filt.shape), pw, ph))
    marks, first, map_of = demo_marks(VD, CP)
    atlas, _ = demo_atlas()
    shape = (ph, 5 * pw, 3)
    chunk = max(1, min(int(chunk), _MAX_CHUNK, _RING_BYTES // int(np.prod(shape))))
    result = None
    if sink is None:
        result = np.empty((fc,) + shape, np.uint8)

        def sink(c, _pos=[0]):
            result[_pos[0]:_pos[0] + c.shape[0]] = c
            _pos[0] += c.shape[0]
    if fc == 0:
        return result
    import torch
    from . import ops, smartVidCrop as S
    engine = engine or S.get_engine()
    dev = engine.device
    marks_d, first_d, map_d, atlas_d = (torch.from_numpy(a).to(dev) for a in (marks, first, map_of, atlas))    # (once per video)
    out = _OutRing(engine, chunk, ph, 5 * pw, sink)
    cap = out.ring['key'][0]

    def consume(staged, s):
        for a in range(s, s + int(staged.shape[0]), cap):      # (a host feed stages at most 32 frames, the ring holds `chunk`)
            part = staged[a - s:a - s + cap]
            k = int(part.shape[0])
            small = engine.resize_frames(part, ph, pw, src.pix_fmt, src.layout, src.colour)
            # (a chunk's frames name their rows of the video's one mark list: first[a .. a + k])
            out.put(k, lambda dst: ops.demo_frames(small, raw, filt, map_d[a:a + k], marks_d, first_d[a:a + k + 1], atlas_d, bgr, dst))
    src.chunks(engine, fc, chunk, consume)
    out.flush()
    return result
