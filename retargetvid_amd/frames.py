"""Where a video's frames are and how they are read: FrameSource resolves a video dict's (or a bare container's) kind of
container, pixel format and layout once, and reads it for the ingest, shot detection and the renderer; _HostFeed is the
pinned, double-buffered staging of frames that live in host memory."""
import numpy as np

_STAGE_BYTES = 96 << 20        # pinned / device staging buffer size of the host-fed ingest (two of each per engine)


class _HostFeed:
    """Host frames -> saliency-size frames on the device, selection applied BEFORE the copy, with the copies off the
    critical path: two pinned host buffers and two device buffers per engine, H2D on a side stream, the down-scale
    (svc_resize_frames_u8) on the caller's stream.  While chunk c is being copied and down-scaled the host gathers
    chunk c+1 into the other pinned buffer; an event per buffer keeps a pinned slot from being refilled before its
    copy has run and a device slot from being overwritten before its down-scale has read it.  Replaces the reference's
    per-frame cv2.resize on the host inside the read loop (smartVidCrop.py:333-335, :633-635) for inputs that live in
    host memory; the 4K stream of BASELINE config 5 is bound by this copy (24.9 MB per frame over PCIe as RGB, 12.4 MB as
    NV12: the staging is sized by the frame's bytes, whatever its format)."""

    def __init__(self, engine):
        import torch
        self.engine = engine
        self.dev = engine.device
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.shape = None

    def _buffers(self, shape):
        """Staging for frames of `shape` ((h, w, 3) RGB or (h * 3 / 2, w) NV12: the shape tells the format)."""
        import torch
        if self.shape != shape:
            k = max(1, min(32, _STAGE_BYTES // int(np.prod(shape))))
            self.pinned = [torch.empty((k,) + shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.staged = [torch.empty((k,) + shape, dtype=torch.uint8, device=self.dev) for _ in range(2)]
            self.copied = [torch.cuda.Event(), torch.cuda.Event()]       # H2D of the slot has run
            self.consumed = [torch.cuda.Event(), torch.cuda.Event()]     # the down-scale has read the device slot
            self.used = [False, False]
            self.shape, self.k = shape, k
        return self.k

    def downscale(self, frames, idx, sal_h, sal_w, pix_fmt='rgb24', layout=None, colour=None):
        """frames: host frames [n,h,w,3] u8 (pix_fmt='nv12': [n,h*3/2,w]; with a layout: [n, frame_stride], staged as they are
        and read through the layout on the device, no host repack) -- a numpy array (pageable memory: gathered into
        the pinned slots by a few threads) or a PINNED torch tensor (copied from where it lies, frame by frame); idx: selected
        frame numbers; colour: of nv12 frames (Engine.resize_frames').  -> uint8 CUDA tensor [len(idx), sal_h, sal_w, 3] RGB, produced
        on the caller's current stream."""
        import torch
        out = torch.empty((len(idx), sal_h, sal_w, 3), dtype=torch.uint8, device=self.dev)

        def put(staged, s):
            out[s:s + staged.shape[0]] = self.engine.resize_frames(staged, sal_h, sal_w, pix_fmt, layout, colour)
        self.feed(frames, idx, put)
        return out

    def feed(self, frames, idx, consume):
        """The staging loop behind downscale (and render.render_video): frames idx of a host container reach the device in
        chunks of at most k frames; consume(staged_chunk, s) enqueues the chunk's device work on the caller's current
        stream (staged_chunk: uint8 CUDA [m, *frame shape], valid until that work has run; s: position of its first frame in idx)."""
        import torch
        shape = tuple(int(v) for v in frames.shape[1:])
        nbytes = int(np.prod(shape))
        k = self._buffers(shape)
        compute = torch.cuda.current_stream(self.dev)
        direct = torch.is_tensor(frames) and frames.is_pinned()
        src = frames if direct else (frames.numpy() if torch.is_tensor(frames) else frames)
        for c, s in enumerate(range(0, len(idx), k)):
            part = idx[s:s + k]
            slot = c & 1
            if self.used[slot] and not direct:
                self.copied[slot].synchronize()                 # the pinned slot's previous copy has run
            if not direct:                                      # selection before the copy: only these frames cross PCIe
                host = self.pinned[slot].numpy()
                if len(part) > 1 and nbytes >= (1 << 20):       # big frames: the gather itself is the bottleneck (one thread
                    list(self._pool().map(lambda jf: np.copyto(host[jf[0]], src[jf[1]]), enumerate(part)))   # copies ~10 GB/s)
                else:
                    np.take(src, part, axis=0, out=host[:len(part)], mode='clip')
            with torch.cuda.stream(self.copy_stream):
                if self.used[slot]:
                    self.copy_stream.wait_event(self.consumed[slot])    # the device slot's previous reader is done
                if direct:
                    if len(part) > 1 and part[-1] - part[0] == len(part) - 1 and all(part[j + 1] == part[j] + 1 for j in range(len(part) - 1)):
                        self.staged[slot][:len(part)].copy_(src[part[0]:part[0] + len(part)], non_blocking=True)     # a run of consecutive frames: one copy
                    else:
                        for j, f in enumerate(part):
                            self.staged[slot][j].copy_(src[f], non_blocking=True)
                else:
                    self.staged[slot][:len(part)].copy_(self.pinned[slot][:len(part)], non_blocking=True)
                self.copied[slot].record(self.copy_stream)
            compute.wait_event(self.copied[slot])
            consume(self.staged[slot][:len(part)], s)
            self.consumed[slot].record(compute)
            self.used[slot] = True

    def _pool(self):
        if getattr(self, '_tp', None) is None:
            from concurrent.futures import ThreadPoolExecutor
            self._tp = ThreadPoolExecutor(max_workers=4)
        return self._tp


def device_index(engine, idx, dev=None):
    """Frame numbers -> int64 CUDA tensor WITHOUT a host-device synchronisation: torch.as_tensor(list, device=...) copies from
    pageable memory, i.e. waits for everything the stream holds -- once per read batch that is the end of the host's run-ahead
    (and, with several videos in flight, of their overlap).  An arithmetic progression is generated on the device; any
    other list travels through a small ring of pinned slots (an event per slot: a slot is not refilled before its copy ran)."""
    import torch
    dev = dev or engine.device
    n = len(idx)
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=dev)
    step = int(idx[1]) - int(idx[0]) if n > 1 else 1
    if step > 0 and all(int(idx[i + 1]) - int(idx[i]) == step for i in range(n - 1)):
        return torch.arange(int(idx[0]), int(idx[0]) + step * n, step, dtype=torch.int64, device=dev)
    ring = engine.__dict__.get('_idx_ring')
    if ring is None or ring['cap'] < n or ring['dev'] != dev:
        cap = max(4096, n)
        ring = engine.__dict__['_idx_ring'] = dict(cap=cap, dev=dev, k=0, host=[torch.empty(cap, dtype=torch.int64).pin_memory() for _ in range(4)],
                                                   ev=[None] * 4)
    k = ring['k'] = (ring['k'] + 1) & 3
    if ring['ev'][k] is not None:
        ring['ev'][k].synchronize()
    host = ring['host'][k]
    host[:n] = torch.as_tensor(np.asarray(idx, dtype=np.int64))
    out = host[:n].to(dev, non_blocking=True)
    ev = ring['ev'][k] = ring['ev'][k] or torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    return out


def _runs(idx):
    """Frame numbers, in order, as runs with a constant positive step: [(first, count, step)], greedily from the left, so that
    each run is the strided view frames[first : first + (count - 1) * step + 1 : step].  A frame that continues no run (a
    repeat, a step backwards, the last one) is a run of one with step 1."""
    idx = [int(v) for v in idx]
    runs, s = [], 0
    while s < len(idx):
        step = idx[s + 1] - idx[s] if s + 1 < len(idx) else 0
        e = s + 1
        while step > 0 and e < len(idx) and idx[e] - idx[e - 1] == step:
            e += 1
        runs.append((idx[s], e - s, step if e - s > 1 else 1))
        s = e
    return runs


def _is_run(idx):
    """idx is one run of consecutive frame numbers (a range says so itself; a list is walked only when its ends fit)."""
    if isinstance(idx, range):
        return len(idx) > 0 and idx.step == 1
    n = len(idx)
    return n > 0 and int(idx[-1]) - int(idx[0]) == n - 1 and all(int(idx[i + 1]) - int(idx[i]) == 1 for i in range(n - 1))


class FrameSource:
    """What holds a video's frames and how each kind of holder is read: resolved ONCE per video by FrameSource.of, without
    device work, and asked for frames by the ingest (small), shot detection (small) and the renderer (chunks).

    kind       the container
    ---------  -------------------------------------------------------------------------------------------------------
    device     a CUDA tensor: read where it lies (no copy when it is on the engine's device)
    host       a numpy array, anything numpy reads, or a host tensor that is not pinned: the selected frames are gathered
               into pinned double buffers, H2D on a side stream (_HostFeed)
    pinned     a pinned torch tensor: copied from where it lies, frame by frame or run by run (_HostFeed)
    generator  an object with __len__, h, w and select(idx) -> uint8 CUDA frames (synth.LazyBlobVideo): frames on demand
    selected   only the frames the ingest will select, in pinned memory: .pinned and .rows(idx) (synth.HostSelectedVideo)
    None       a dict whose 'frames' is None (an analysed video whose frames are gone: the feature cache still reads key())

    frames: the container (np.asarray of what is neither a tensor nor one of the two objects); pix_fmt 'rgb24' (uint8
    [n, h, w, 3]) or 'nv12' (uint8 [n, h * 3 / 2, w]); layout: None for such packed frames, else the checked ops.FrameLayout
    of uint8 [n, frame_stride] frames as a decoder left them (device, host, pinned and selected); n frames of an h x w PICTURE;
    colour: the (matrix, range) nv12 frames are decoded with (ops.frame_colour's; ('bt601', 'limited') unless the video says
    otherwise), None for rgb24, which has none."""
    __slots__ = ('kind', 'frames', 'pix_fmt', 'layout', 'n', 'h', 'w', 'colour')

    @classmethod
    def of(cls, video, pix_fmt=None, layout=None, colour=None):
        """video: an ingest_pickle dict (frames, w, h, and optionally pix_fmt and layout=dict(pitch=, chroma_offset=,
        chroma_pitch=) or an ops.FrameLayout, and colour=dict(matrix='bt709', range='full'), missing keys 'bt601' / 'limited'), a bare
        container, or a FrameSource (returned as it is).  pix_fmt / layout / colour
        describe a bare container; a dict's own entries win.  A packed dict without h / w takes them from the container's shape.
        Every refusal is raised here, before any device work: ValueError for an unknown format, an NV12 picture of odd size, a
        container of another shape, a broken rule of ops.frame_layout, a layout on a generator, an unknown colour matrix or
        range, a colour on rgb24 frames (which have none); TypeError for frames that are not uint8."""
        if isinstance(video, cls):
            return video
        import torch
        from . import ops
        u8 = (np.uint8, torch.uint8)
        is_dict = isinstance(video, dict)
        self = cls()
        frames = video['frames'] if is_dict else video
        lay = video.get('layout') if is_dict and video.get('layout') is not None else layout
        fmt = (is_dict and video.get('pix_fmt')) or pix_fmt or (lay.pix_fmt if isinstance(lay, ops.FrameLayout) else 'rgb24')
        h, w = (video.get('h'), video.get('w')) if is_dict else (None, None)
        col = video.get('colour') if is_dict and video.get('colour') is not None else colour
        if col is not None:
            col = ops.frame_colour(col)
            if fmt == 'rgb24':
                raise ValueError('colour=%r describes nv12 frames; these are rgb24, which are the colours themselves' % (col,))
        if frames is None:
            kind = None
        elif torch.is_tensor(frames):
            kind = 'device' if frames.is_cuda else 'pinned' if frames.is_pinned() else 'host'
        elif hasattr(frames, 'pinned') and hasattr(frames, 'rows'):
            kind = 'selected'
        elif hasattr(frames, 'select') and not hasattr(frames, 'shape'):
            kind = 'generator'
        else:
            kind, frames = 'host', np.asarray(frames)
        arr = frames.pinned if kind == 'selected' else frames          # what has a shape and a dtype
        shape = tuple(int(v) for v in arr.shape) if kind not in (None, 'generator') else None
        if lay is None and shape is not None:
            if fmt == 'rgb24' and (len(shape) != 4 or shape[3] != 3 or arr.dtype not in u8):
                raise TypeError('frames must be uint8 [n,h,w,3] RGB')
            if fmt == 'nv12' and arr.dtype not in u8:
                raise TypeError('nv12 frames must be uint8 [n,h*3/2,w]')
        if h is None or w is None:
            if kind in ('generator', 'selected'):
                h, w = frames.h, frames.w
            elif isinstance(lay, ops.FrameLayout):
                h, w = lay.h, lay.w
            elif lay is None and shape is not None:
                _, h, w = ops.picture_size(arr, fmt)
        want = ops.frame_shape(fmt, h, w)                              # unknown format, NV12 picture of odd size
        if lay is not None:
            if kind == 'generator':
                raise ValueError('a layout describes frames in memory: %s produces its frames on demand (.select) and takes none'
                                 % type(frames).__name__)
            if shape is not None and len(shape) != 2:
                raise ValueError('frames with a layout are uint8 [n, frame_stride], not %s' % (shape,))
            stride = shape[1] if shape is not None else None
            if isinstance(lay, ops.FrameLayout):
                stride, lay = lay.frame_stride, dict(pitch=lay.pitch, chroma_offset=lay.chroma_offset, chroma_pitch=lay.chroma_pitch)
            lay = ops.frame_layout(fmt, h, w, lay, stride)
            if shape is not None and (arr.dtype not in u8 or shape[1] != lay.frame_stride):
                raise ValueError('frames with this layout are uint8 [n, %d], not %s %s' % (lay.frame_stride, arr.dtype, shape))
        elif shape is not None and fmt != 'rgb24' and shape[1:] != want:
            raise ValueError('%s frames of a %d x %d picture are uint8 [n, %s], not %s' % (fmt, w, h, ', '.join(str(v) for v in want), shape))
        self.kind, self.frames, self.pix_fmt, self.layout = kind, frames, fmt, lay
        self.colour = (col or ops.DEFAULT_COLOUR) if fmt == 'nv12' else None
        self.n = None if kind is None else len(frames) if shape is None or kind == 'selected' else shape[0]
        self.h, self.w = int(h), int(w)
        return self

    def key(self):
        """The feature cache's entries for the format, -- for frames with a layout -- where their bytes lie, and -- for nv12 frames
        that are not BT.601 limited -- their colour: features computed under one colour are never read under another."""
        from .ops import DEFAULT_COLOUR
        key = dict(pix_fmt=self.pix_fmt)
        if self.colour not in (None, DEFAULT_COLOUR):
            key['colour'] = self.colour
        if self.layout is not None:
            key['layout'] = self.layout.key()
        return key

    def whole(self):
        """self, if every frame of the video can be read (what chunks needs)."""
        if self.kind == 'selected':
            raise ValueError('render_video needs every frame of the video; %s holds only the frames the ingest selected'
                             % type(self.frames).__name__)
        return self

    def small(self, engine, idx, sh, sw):
        """Frames idx (a list or a range; any order, repeats allowed) at sh x sw as RGB -> uint8 CUDA [len(idx), sh, sw, 3] on the engine's device,
        produced on the current stream."""
        import torch
        dev, frames, fmt, lay, col = engine.device, self.frames, self.pix_fmt, self.layout, self.colour
        if self.kind == 'device':
            if frames.device != dev:               # gathered where the container lies, then moved
                return engine.resize_frames(frames[device_index(engine, idx, frames.device)].to(dev).contiguous(), sh, sw, fmt, lay, col)
            if lay is None:
                # one run of consecutive frames is a slice of the container; any other selection is gathered with a device index
                if _is_run(idx):
                    return engine.resize_frames(frames[int(idx[0]):int(idx[0]) + len(idx)].contiguous(), sh, sw, fmt, None, col)
                return engine.resize_frames(frames[device_index(engine, idx, dev)].contiguous(), sh, sw, fmt, None, col)
            # nothing is gathered: a selection with a constant step (consecutive frames, or every skip-th: what the ingest selects)
            # is one strided view, read with a frame stride of step surfaces; any other selection is cut into such runs
            small = [engine.resize_frames(frames[first:first + (count - 1) * step + 1:step], sh, sw, fmt, lay if step == 1 else lay.every(step), col)
                     for first, count, step in _runs(idx)]
            return small[0] if len(small) == 1 else torch.cat(small) if small else torch.empty((0, sh, sw, 3), dtype=torch.uint8, device=dev)
        if self.kind == 'generator':
            if getattr(frames, 'accepts_device_index', False):
                sel = frames.select(idx, index=device_index(engine, idx, dev))
            else:
                sel = frames.select(idx)
            return engine.resize_frames(sel.to(dev).contiguous(), sh, sw, fmt, None, col)
        feed = getattr(engine, '_host_feed', None)
        if feed is None:
            feed = engine._host_feed = _HostFeed(engine)
        if self.kind == 'selected':
            return feed.downscale(frames.pinned, frames.rows(idx), sh, sw, fmt, lay, col)
        return feed.downscale(frames, idx, sh, sw, fmt, lay, col)

    def chunks(self, engine, count, chunk, consume):
        """The first `count` frames, in order and at full size, as staged chunks on the engine's device: consume(staged, s)
        enqueues a chunk's device work on the current stream (staged: uint8 CUDA [m, *frame shape], valid until that work has
        run; s: number of its first frame).  A generator and a device container give chunks of `chunk` frames; a host container
        gives what its staging holds (at most 32)."""
        import torch
        dev, frames = engine.device, self.whole().frames
        if self.kind == 'generator':
            for s in range(0, count, chunk):
                consume(frames.select(range(s, min(count, s + chunk))).to(dev).contiguous(), s)
        elif self.kind == 'device':
            src = frames if frames.device == dev else frames[:count].to(dev)
            src = src.contiguous()                 # (frames with a layout are [n, frame_stride] rows: nothing is repacked)
            for s in range(0, count, chunk):
                consume(src[s:min(count, s + chunk)], s)
        else:
            feed = engine.__dict__.get('_render_feed')
            if feed is None:
                feed = engine._render_feed = _HostFeed(engine)          # its own staging (the ingest's keeps its size)
            feed.feed(frames, list(range(count)), consume)
