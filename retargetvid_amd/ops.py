"""Device operators of the hot path (torch tensors in, torch tensors out).

Thin wrappers over the C ABI (include/svc.h): PyTorch is used only for device memory and
streams.  Every function requires a GPU and the built HIP library — nothing here has a
CPU path."""
import ctypes

import numpy as np
import torch

from . import _lib, weights as _weights
from ._lib import SvcParams

TAP_INPUT, TAP_FEAT4X, TAP_FEAT2X, TAP_FEAT1X, TAP_POSTCNN, TAP_DEC, TAP_PRE = range(7)
# nodes of svc_debug_run_node (include/svc.h: SVC_NODE_*); backbone block idx = 2 .. 17 is node idx
NODE_FRONT, NODE_F18, NODE_SKIP_2X, NODE_SKIP_4X, NODE_POST_CNN, NODE_US2, NODE_POST_US2, NODE_ADAPT, NODE_SMOOTH = 1, 18, 19, 20, 21, 22, 23, 24, 25
NODE_F4X, NODE_F2X = 107, 114
NODE_MAP, NODE_MAP_PROFILE = 26, 27     # logits -> [2, h, w]: the pre-softmax map and the uint8 map's values (k_quantise / k_quantise_profile)


# words of svc_debug_net_plan (include/svc.h: SVC_PLAN_*), in order
PLAN_WORDS = ('NH', 'NW', 'hks', 'vks', 'fr_ok', 'fr_nr', 'fr_nc', 'fr_tiles_y', 'fr_tiles_x', 'lz_tile_cap', 'lz_lds', 'sd_rows',
              'sd_tile_cap', 'sd_lds', 'fr_lds', 'lz_lds_max', 'sd_lds_max', 'fr_lds_max')

# words of svc_debug_tail_plan (include/svc.h: SVC_TAILPLAN_*), in order
TAIL_PLAN_WORDS = ('h', 'w', 'fused', 'lvl_big', 'tree_fallback', 'cap_cl', 'cap_cl_huge', 'LVL_CAP', 'TP_CAP', 'TP_CAP_BIG', 'TREE_LDS_CAP',
                   'TREE_LDS_CLUSTERS', 'n_ring', 'n_ring1', 'RING_R', 'RING_R1', 'CORE_REG_STEP', 'CORE_REG_MAX', 'core_lds_max')

# words of svc_debug_sort_plan (include/svc.h: SVC_SORTPLAN_*), in order
SORT_PLAN_WORDS = ('in_lds', 'nseg', 'depth', 'lds_bytes')

# words of a frame header, cluster_state(...)['hdr'] (include/svc.h: SVC_HDR_*, the same numbers; a range is its first word and a count)
HDR_WORDS = 32
HDR_N, HDR_NSEL, HDR_KEPT, HDR_CLUSTERED, HDR_NCLUSTERS = 0, 1, 2, 3, 4
HDR_CORE_STAMP0, HDR_CORE_STAMPS = 5, 3
HDR_T_SORTED, HDR_T_HIERARCHY, HDR_T_CHOSEN, HDR_T_FINISHED, HDR_T_PRIM, HDR_T_BUILT = 8, 9, 10, 11, 12, 13
HDR_TREE_CLOCKS, HDR_T_TREE = 14, 15
HDR_LVL_ROUNDS, HDR_LVL_RISES = 16, 17
HDR_LVL_PHASE0, HDR_LVL_PHASES = 18, 5
HDR_TREE_PAR, HDR_T_LVL_SETUP = 23, 24
HDR_TP_STAMP0, HDR_TP_STAMPS = 25, 5
HDR_BACK_DONE = 30


def net_plan(height, width):
    """Test door (svc_debug_net_plan): what the network's plan decides from the map shape alone, as a dict of PLAN_WORDS.  Host
    arithmetic of the library: needs no GPU."""
    out = (ctypes.c_int32 * len(PLAN_WORDS))()
    n = _lib.check(_lib.load().svc_debug_net_plan(int(height), int(width), ctypes.cast(out, ctypes.c_void_p), len(PLAN_WORDS)))
    if n != len(PLAN_WORDS):
        raise _lib.SvcError('svc_debug_net_plan reports %d words, this binding knows %d' % (n, len(PLAN_WORDS)))
    return dict(zip(PLAN_WORDS, (int(v) for v in out)))


def sort_plan(n):
    """Test door (svc_debug_sort_plan): what the edge sort (k_sort, Engine.argsort_u32) decides from the number of keys alone, as a
    dict of SORT_PLAN_WORDS -- 'in_lds': the working arrays are in LDS (0: in global scratch), 'nseg', 'depth' (the depth limit,
    2 * floor(log2 n)), 'lds_bytes'.  The function the kernels carve their arrays by, run on the host: needs no GPU."""
    lib = _lib.load()
    if not hasattr(lib, 'svc_debug_sort_plan'):
        raise _lib.SvcError('%s lacks svc_debug_sort_plan: the plan door of the edge sort needs a build that has it' % _lib.LIB_PATH)
    out = (ctypes.c_int32 * len(SORT_PLAN_WORDS))()
    got = _lib.check(lib.svc_debug_sort_plan(int(n), ctypes.cast(out, ctypes.c_void_p), len(SORT_PLAN_WORDS)))
    if got != len(SORT_PLAN_WORDS):
        raise _lib.SvcError('svc_debug_sort_plan reports %d words, this binding knows %d' % (got, len(SORT_PLAN_WORDS)))
    return dict(zip(SORT_PLAN_WORDS, (int(v) for v in out)))


def scratch_fill(byte):
    """Test door (svc_debug_scratch_fill), process-wide: byte 0..255 = every pass of every handle fills its scratch workspaces with that
    byte before its first kernel (the tail's index workspace with zeros); None = off, the default.  For tests: a pass that reads what
    it did not write reads the fill, not what the previous call left.  Needs no GPU to set."""
    _lib.check(_lib.load().svc_debug_scratch_fill(-1 if byte is None else int(byte)))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _need_cuda(t, dtype, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError('%s must be a contiguous CUDA tensor of dtype %s' % (name, dtype))


RENDER_BGR = 1                       # svc_render_crops_u8 flag (include/svc.h: SVC_RENDER_BGR)
PIX_FMTS = ('rgb24', 'nv12')         # input pixel formats: uint8 [n,h,w,3] RGB | uint8 [n,h*3/2,w] (include/svc.h: the _nv12 entries)
OUT_FMTS = ('rgb24', 'nv12')         # the renderer's output formats: the same two shapes (include/svc.h: the _to_nv12 entries)
INTERPS = ('linear', 'lanczos')      # the renderer's resampling filters (include/svc.h: SVC_FILTER_*, by index)
RENDER_ENTRIES = {('rgb24', 'rgb24'): 'svc_render_crops_u8', ('nv12', 'rgb24'): 'svc_render_crops_nv12',        # (pix_fmt, out_fmt)
                  ('rgb24', 'nv12'): 'svc_render_crops_u8_to_nv12', ('nv12', 'nv12'): 'svc_render_crops_nv12_to_nv12'}


MATRICES = ('bt601', 'bt709')        # the colour matrices of NV12 frames (include/svc.h: SVC_MATRIX_*, by index)
RANGES = ('limited', 'full')         # and their ranges (include/svc.h: SVC_RANGE_*, by index)
DEFAULT_COLOUR = ('bt601', 'limited')
# other names the same things go by (libav's colorspace / color_range names), lower case
_MATRIX_NAMES = dict(bt601='bt601', bt470bg='bt601', smpte170m='bt601', bt709='bt709')
_RANGE_NAMES = dict(limited='limited', tv='limited', mpeg='limited', full='full', pc='full', jpeg='full')


def frame_colour(spec):
    """The colour of NV12 frames, checked and normalised -> (matrix, range), one of MATRICES x RANGES.  spec: None (BT.601
    limited), dict(matrix=, range=) with missing keys (or None) taking 'bt601' / 'limited', or a (matrix, range) pair.  Names
    are case-insensitive; 'bt470bg' and 'smpte170m' say bt601, 'tv' / 'mpeg' say limited, 'pc' / 'jpeg' say full.  ValueError for
    an unknown matrix, range or key -- before any device work."""
    if spec is None:
        return DEFAULT_COLOUR
    if isinstance(spec, dict):
        unknown = sorted(set(spec) - {'matrix', 'range'})
        if unknown:
            raise ValueError('unknown colour key %s (the keys are matrix, range)' % ', '.join(map(repr, unknown)))
        matrix, rng = spec.get('matrix'), spec.get('range')
    elif isinstance(spec, (tuple, list)) and len(spec) == 2:
        matrix, rng = spec
    else:
        raise ValueError('a colour is dict(matrix=, range=) or a (matrix, range) pair, not %r' % (spec,))
    m = _MATRIX_NAMES.get(str(matrix).lower()) if matrix is not None else 'bt601'
    r = _RANGE_NAMES.get(str(rng).lower()) if rng is not None else 'limited'
    if m is None:
        raise ValueError('unknown colour matrix %r (one of %s)' % (matrix, ', '.join(MATRICES)))
    if r is None:
        raise ValueError('unknown colour range %r (one of %s)' % (rng, ', '.join(RANGES)))
    return (m, r)


def _side_colour(spec, fmt, what):
    """frame_colour of one side of a call (`what` names the keyword) -> (matrix, range) or None for the default; a colour given
    for an rgb24 side is a ValueError: nothing would read it."""
    if spec is None:
        return None
    c = frame_colour(spec)
    if fmt != 'nv12':
        raise ValueError('%s describes nv12 frames; this side is %s (pass None)' % (what, fmt))
    return None if c == DEFAULT_COLOUR else c


def _colour_struct(c):
    """(matrix, range) -> the SvcColour the C entries take; None -> NULL (BT.601 limited)."""
    if c is None:
        return None
    return ctypes.byref(_lib.SvcColour(ctypes.sizeof(_lib.SvcColour), MATRICES.index(c[0]), RANGES.index(c[1]), 0))


def frame_shape(pix_fmt, h, w):
    """Shape of one frame of a h x w picture in `pix_fmt`; ValueError for an unknown format or an NV12 picture of odd size."""
    h, w = int(h), int(w)
    if pix_fmt == 'rgb24':
        return (h, w, 3)
    if pix_fmt == 'nv12':
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError('an nv12 picture has even width and height (>= 2), not %d x %d' % (w, h))
        return (h * 3 // 2, w)
    raise ValueError('unknown pix_fmt %r (one of %s)' % (pix_fmt, ', '.join(PIX_FMTS)))


def out_frame_shape(out_fmt, oh, ow, bgr=False):
    """Shape of one rendered frame of oh x ow in `out_fmt` (frame_shape's); ValueError for an unknown format, an NV12 output of
    odd size, or bgr with NV12 -- what the renderer's doors check before any device work."""
    if out_fmt not in OUT_FMTS:
        raise ValueError('unknown out_fmt %r (one of %s)' % (out_fmt, ', '.join(OUT_FMTS)))
    if out_fmt == 'nv12':
        if bgr:
            raise ValueError('bgr has no meaning for an nv12 output')
        if oh < 2 or ow < 2 or oh % 2 or ow % 2:
            raise ValueError('an nv12 output has even width and height (>= 2), not %d x %d: pass an even out_size' % (ow, oh))
    return frame_shape(out_fmt, oh, ow)


def check_interp(interp):
    """ValueError unless `interp` is one of INTERPS -- what the renderer's doors check before any device work."""
    if interp not in INTERPS:
        raise ValueError('unknown interp %r (one of %s)' % (interp, ', '.join(INTERPS)))
    return interp


def picture_size(frames, pix_fmt):
    """(n, h, w) of the PICTURES in a frames tensor / array of `pix_fmt`; the shape is checked."""
    shape = tuple(int(v) for v in frames.shape)
    if pix_fmt == 'nv12':
        if len(shape) != 3 or shape[1] % 3 or shape[1] < 3:
            raise ValueError('nv12 frames are uint8 [n, h * 3 / 2, w], not %s' % (shape,))
        n, h, w = shape[0], shape[1] * 2 // 3, shape[2]
    else:
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError('%s frames are uint8 [n, h, w, 3], not %s' % (pix_fmt, shape))
        n, h, w = shape[:3]
    if shape[1:] != frame_shape(pix_fmt, h, w):
        raise ValueError('frames of shape %s are not %s frames' % (shape, pix_fmt))
    return n, h, w


LAYOUT_KEYS = ('pitch', 'chroma_offset', 'chroma_pitch')


class FrameLayout:
    """Where the bytes of a h x w picture's frames lie (include/svc.h: SvcFrameLayout), checked: what frame_layout returns and
    the layout= of Engine.resize_frames / render_crops takes.  extent: bytes from a frame's start to the end of its last plane row."""
    __slots__ = ('pix_fmt', 'h', 'w', 'frame_stride', 'pitch', 'chroma_offset', 'chroma_pitch', 'extent')

    def key(self):
        return (self.pix_fmt, self.h, self.w, self.frame_stride, self.pitch, self.chroma_offset, self.chroma_pitch)

    def __eq__(self, other):
        return isinstance(other, FrameLayout) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'FrameLayout(%s %dx%d frame_stride=%d pitch=%d chroma_offset=%d chroma_pitch=%d)' % (
            self.pix_fmt, self.w, self.h, self.frame_stride, self.pitch, self.chroma_offset, self.chroma_pitch)

    def every(self, step):
        """The layout of every step-th frame of these: the same planes, frames step * frame_stride apart (a strided view
        frames[a::step] of the container is then read where it lies)."""
        L = FrameLayout()
        for k in self.__slots__:
            setattr(L, k, getattr(self, k))
        L.frame_stride = self.frame_stride * int(step)
        return L

    def struct(self):
        """The SvcFrameLayout the C entries take."""
        return _lib.SvcFrameLayout(ctypes.sizeof(_lib.SvcFrameLayout), PIX_FMTS.index(self.pix_fmt), self.frame_stride, self.pitch,
                                   self.chroma_offset, self.chroma_pitch)


def frame_layout(pix_fmt, h, w, layout=None, frame_stride=None):
    """The layout of the frames of a h x w picture in `pix_fmt` -> FrameLayout.  layout: dict(pitch=, chroma_offset=,
    chroma_pitch=) in bytes, missing keys (or None) taking their packed value (pitch 3 w | w, chroma_offset pitch * h,
    chroma_pitch = pitch; both chroma values 0 for rgb24); frame_stride: bytes from frame to frame (None: the frame's extent, i.e. no
    gap).  ValueError with the rule of include/svc.h that is broken -- the checks the C launchers make, made before any device work."""
    shape = frame_shape(pix_fmt, h, w)
    h, w = int(h), int(w)
    layout = dict(layout or {})
    unknown = sorted(set(layout) - set(LAYOUT_KEYS))
    if unknown:
        raise ValueError('unknown layout key %s (the keys are %s)' % (', '.join(map(repr, unknown)), ', '.join(LAYOUT_KEYS)))
    nv12 = pix_fmt == 'nv12'
    row = w if nv12 else 3 * w
    L = FrameLayout()
    L.pix_fmt, L.h, L.w = pix_fmt, h, w
    L.pitch = int(layout['pitch']) if layout.get('pitch') is not None else row
    if nv12:
        L.chroma_offset = int(layout['chroma_offset']) if layout.get('chroma_offset') is not None else L.pitch * h
        L.chroma_pitch = int(layout['chroma_pitch']) if layout.get('chroma_pitch') is not None else L.pitch
    else:
        L.chroma_offset, L.chroma_pitch = int(layout.get('chroma_offset') or 0), int(layout.get('chroma_pitch') or 0)
    if min(L.pitch, L.chroma_offset, L.chroma_pitch, 0 if frame_stride is None else int(frame_stride)) < 0:
        raise ValueError('layout values must be non-negative')
    if L.pitch < row:
        raise ValueError("pitch %d is below the row's %d bytes" % (L.pitch, row))
    if not nv12 and (L.chroma_offset or L.chroma_pitch):
        raise ValueError('chroma_offset and chroma_pitch must be 0 for rgb24')
    if nv12 and L.chroma_pitch < w:
        raise ValueError('chroma_pitch %d is below the width %d' % (L.chroma_pitch, w))
    if nv12 and L.chroma_offset < L.pitch * (h - 1) + w:
        raise ValueError('chroma_offset %d is below pitch * (height - 1) + width = %d: the chroma plane overlaps the last luma row'
                         % (L.chroma_offset, L.pitch * (h - 1) + w))
    L.extent = L.chroma_offset + L.chroma_pitch * (h // 2 - 1) + w if nv12 else L.pitch * (h - 1) + 3 * w
    L.frame_stride = L.extent if frame_stride is None else int(frame_stride)
    if L.frame_stride < L.extent:
        raise ValueError("frame_stride %d is below the frame's extent of %d bytes" % (L.frame_stride, L.extent))
    if max(L.key()[3:]) >= 1 << 62:
        raise ValueError('layout values must be below 2^62')
    assert layout or frame_stride is not None or L.extent == int(np.prod(shape))
    return L


def _pitched(frames, layout, pix_fmt, what='frames'):
    """frames of a FrameLayout: a uint8 CUDA tensor [n, frame_stride] -- or any 2-D view with unit element stride whose rows are
    frame_stride bytes apart and hold the frame's extent (the last frame need not have its trailing gap) -> n.  what: the
    keyword the errors name ('frames'; 'out' for an output with an out_layout, which lies under the same rules)."""
    if not isinstance(layout, FrameLayout):
        raise TypeError('%s must be an ops.FrameLayout (ops.frame_layout(pix_fmt, h, w, dict(pitch=...), frame_stride))'
                        % ('layout' if what == 'frames' else 'out_layout'))
    if layout.pix_fmt != pix_fmt:
        raise ValueError('the layout is one of %s frames, %s says %s' % (layout.pix_fmt, 'pix_fmt' if what == 'frames' else 'out_fmt', pix_fmt))
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
        raise TypeError('%s must be a CUDA tensor of dtype torch.uint8' % what)
    if frames.dim() != 2:
        raise ValueError('%s with a layout are uint8 [n, frame_stride], not %s' % (what, tuple(frames.shape),))
    n = int(frames.shape[0])
    if n and (frames.stride(1) != 1 or int(frames.shape[1]) < layout.extent or (n > 1 and frames.stride(0) != layout.frame_stride)):
        raise ValueError('%s of shape %s and strides %s do not hold frames of %d bytes that lie %d bytes apart'
                         % (what, tuple(frames.shape), tuple(frames.stride()), layout.extent, layout.frame_stride))
    return n


def out_layout_of(out_layout, out_fmt, oh, ow, frame_stride=None):
    """The layout of an output of oh x ow in `out_fmt`, checked -> FrameLayout (None stays None).  out_layout: an
    ops.FrameLayout, which must be one of that format and picture size, or dict(pitch=, chroma_offset=, chroma_pitch=) (frames
    `frame_stride` apart; None: their extent), resolved by frame_layout.  ValueError with the broken rule -- what the renderer's
    doors check before any device work."""
    if out_layout is None:
        return None
    if isinstance(out_layout, FrameLayout):
        if out_layout.pix_fmt != out_fmt:
            raise ValueError('out_layout is one of %s frames, out_fmt says %s' % (out_layout.pix_fmt, out_fmt))
        if (out_layout.h, out_layout.w) != (int(oh), int(ow)):
            raise ValueError('out_layout is one of %d x %d pictures, the output is %d x %d' % (out_layout.w, out_layout.h, ow, oh))
        return out_layout
    if not isinstance(out_layout, dict):
        raise ValueError('out_layout is an ops.FrameLayout or dict(pitch=, chroma_offset=, chroma_pitch=), not %r' % (out_layout,))
    try:
        return frame_layout(out_fmt, oh, ow, out_layout, frame_stride)
    except ValueError as e:
        raise ValueError('out_layout: %s' % e) from None


def _pictures(frames, layout, pix_fmt):
    """(n, h, w) of the pictures in `frames`, checked: a contiguous CUDA tensor of picture_size's shapes, or, with a layout, what
    _pitched takes."""
    if layout is None:
        _need_cuda(frames, torch.uint8, 'frames')
        return picture_size(frames, pix_fmt)
    return _pitched(frames, layout, pix_fmt), layout.h, layout.w


def _src_args(handle, frames, layout, pix_fmt, n, h, w, *in_colour):
    """The leading arguments of the C entries that take the frames' SvcFrameLayout (and, behind it, in_colour): packed frames
    go as the packed layout's values."""
    lay = (layout or frame_layout(pix_fmt, h, w)).struct()
    return (handle, _ptr(frames), ctypes.byref(lay)) + in_colour + (n, h, w)


def _out_shape(n, out_fmt, oh, ow, bgr, out_layout):
    """Shape of the renderer's output of n frames of oh x ow in `out_fmt`: (n,) + out_frame_shape's, or (n, frame_stride) with an
    out_layout, which must be an ops.FrameLayout (TypeError) of that format and picture size (out_layout_of's ValueErrors)."""
    shape = (n,) + out_frame_shape(out_fmt, oh, ow, bgr)
    if out_layout is not None:
        if not isinstance(out_layout, FrameLayout):
            raise TypeError('out_layout must be an ops.FrameLayout (ops.frame_layout(out_fmt, oh, ow, dict(pitch=...), frame_stride))')
        shape = (n, out_layout_of(out_layout, out_fmt, oh, ow).frame_stride)
    return shape


BLEND_NEXT, MAP_HELD = 1, 2          # bits of cluster_center_'s per-map flags (include/svc.h: SVC_BLEND_NEXT, SVC_MAP_HELD)


class Engine:
    """Owns one SvcHandle (weights + workspace) on one GPU.  Replaces the reference's module-level
    ``unisal_model`` singleton (smartVidCrop.py:77).  Not re-entrant, like the reference."""

    def __init__(self, state_dict=None, device=None, seed=0):
        if not torch.cuda.is_available():
            raise _lib.SvcError('no GPU visible: the SmartVidCrop hot path runs on the MI355X only')
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        if state_dict is None:
            state_dict = _weights.make_synthetic_state_dict(seed)
        self._create(_weights.pack_blob(_weights.fold_state_dict(state_dict)))

    @classmethod
    def from_layers(cls, layers, device=None):
        """A handle from a folded layer list (weights.fold_state_dict's; serialised by weights.pack_blob): the caller chooses the
        numbers the device computes with, without a checkpoint whose BatchNorm folding would have to produce them."""
        if not torch.cuda.is_available():
            raise _lib.SvcError('no GPU visible: the SmartVidCrop hot path runs on the MI355X only')
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self._create(_weights.pack_blob(layers))
        return self

    def _create(self, blob):
        import zlib
        self.weights_id = zlib.crc32(blob) & 0xffffffff        # identifies the checkpoint (smartVidCrop's feature cache keys on it)
        self._h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        _lib.check(self.lib.svc_create(buf, len(blob), self.device.index, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.svc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ingest down-scale -------------------------------------------------------------
    def resize_frames(self, frames, sh, sw, pix_fmt='rgb24', layout=None, colour=None):
        """uint8 [n,h,w,3] -> uint8 [n,sh,sw,3], cv2.resize(INTER_LINEAR) semantics.  pix_fmt='nv12': frames uint8
        [n,h*3/2,w], converted to RGB inside the kernel (svc_resize_frames_nv12): the bytes of the RGB call on the converted frames.
        layout (an ops.FrameLayout): frames uint8 [n, frame_stride] as a decoder left them (svc_resize_frames_layout): the
        bytes of the packed call on the packed pictures, without a repacking pass.
        colour (what ops.frame_colour takes; nv12 only, else ValueError): the matrix and range the frames are decoded with
        (svc_resize_frames_colour); None, or BT.601 limited spelled out, is the call without it."""
        colour = _side_colour(colour, pix_fmt, 'colour')
        n, h, w = _pictures(frames, layout, pix_fmt)
        out = torch.empty((n, sh, sw, 3), dtype=torch.uint8, device=frames.device)
        if colour is not None:              # one entry for every layout: packed frames as the packed layout's values
            lay = (layout or frame_layout(pix_fmt, h, w)).struct()
            entry, src = 'svc_resize_frames_colour', (ctypes.byref(lay), _colour_struct(colour))
        elif layout is not None:
            lay = layout.struct()
            entry, src = 'svc_resize_frames_layout', (ctypes.byref(lay),)
        else:
            entry, src = 'svc_resize_frames_nv12' if pix_fmt == 'nv12' else 'svc_resize_frames_u8', ()
        _lib.check(getattr(self.lib, entry)(self._h, _ptr(frames), *src, n, h, w, _ptr(out), sh, sw, _stream()))
        return out

    # -- rendering ------------------------------------------------------------------------
    def render_crops(self, frames, boxes, out_hw=None, bgr=False, out=None, pix_fmt='rgb24', out_fmt='rgb24', layout=None, interp='linear',
                     colour=None, out_colour=None, out_layout=None):
        """uint8 [n,h,w,3] frames on the device (pix_fmt='nv12': uint8 [n,h*3/2,w], svc_render_crops_nv12; the crops are RGB / BGR
        either way) and int32 [n,4] boxes (x1,y1,x2,y2, one window size for all; a CUDA tensor, or
        host values that are copied over) -> uint8
        [n,oh,ow,3]: frame[y1:y2, x1:x2] copied (out_hw None or the window size) or resampled to out_hw = (oh, ow) with
        cv2.resize(INTER_LINEAR) semantics; bgr: R and B swapped.  Runs on the current stream (svc_render_crops_u8).
        out_fmt='nv12': the crops come out as NV12 frames uint8 [n,oh*3/2,ow] (BT.601 limited range of the RGB crop, fused
        into the kernels: svc_render_crops_u8_to_nv12 / _nv12_to_nv12); oh and ow must be even and bgr unset (ValueError).
        layout (an ops.FrameLayout): frames uint8 [n, frame_stride] as a decoder left them (svc_render_crops_layout); the
        crops are the packed call's on the packed pictures.
        interp='lanczos': resampled as PIL.Image.resize(LANCZOS) does it instead, bit for bit, window cropped first
        (svc_render_crops_filter; include/svc.h states the arithmetic); the window size is the exact copy either way.  Any
        value outside ops.INTERPS: ValueError.
        colour / out_colour (what ops.frame_colour takes): the matrix and range nv12 frames are decoded with / an nv12 output
        is encoded with, chosen independently (svc_render_crops_colour; include/svc.h states the table); None is BT.601
        limited, and the call it always was.  A colour given for an rgb24 side: ValueError.
        out_layout (an ops.FrameLayout of the out_fmt picture of oh x ow: ops.frame_layout(out_fmt, oh, ow, dict(pitch=...),
        frame_stride)): the crops are written where an encoder's surfaces want them (svc_render_crops_to_layout) -> uint8
        [n, frame_stride].  The picture bytes are those of the call without it; no other byte is written (without out= they are
        whatever the allocation held).  out= may be the caller's own 2-D view -- unit element stride, rows frame_stride bytes
        apart that hold the frame's extent, e.g. pool[first:first + n * k:k] of a surface pool: the door for an encoder on the
        same GPU.  A layout of another format or picture size: ValueError before any device work."""
        check_interp(interp)
        _side_colour(colour, pix_fmt, 'colour')
        _side_colour(out_colour, out_fmt if out_fmt in OUT_FMTS else 'nv12', 'out_colour')      # (an unknown out_fmt is reported as that, below)
        n = int(frames.shape[0])
        on_dev = torch.is_tensor(boxes) and boxes.is_cuda
        if n:
            b0 = boxes[0].tolist() if on_dev else np.asarray(boxes)[0].tolist()     # the window size (on_dev: a host read of 16 bytes)
        else:
            b0 = [0, 0, 2, 2] if out_fmt == 'nv12' else [0, 0, 1, 1]
        bw, bh = int(b0[2] - b0[0]), int(b0[3] - b0[1])
        oh, ow = (bh, bw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        shape = _out_shape(n, out_fmt, oh, ow, bgr, out_layout)   # (the ValueErrors come before anything touches the device)
        if layout is None:
            _need_cuda(frames, torch.uint8, 'frames')
        else:
            _pitched(frames, layout, pix_fmt)
        if not on_dev:
            boxes = torch.from_numpy(np.ascontiguousarray(boxes, np.int32)).to(frames.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        return self._render(frames, boxes, bw, bh, out, bgr, pix_fmt, out_fmt, layout, interp, colour, out_colour, out_layout)

    def _render(self, frames, boxes, bw, bh, out, bgr, pix_fmt='rgb24', out_fmt='rgb24', layout=None, interp='linear', colour=None,
                out_colour=None, out_layout=None):
        check_interp(interp)
        colour, out_colour = _side_colour(colour, pix_fmt, 'colour'), _side_colour(out_colour, out_fmt, 'out_colour')
        _need_cuda(boxes, torch.int32, 'boxes')
        if out_layout is not None:          # out: [n, frame_stride] or a view like it
            oh, ow = out_layout.h, out_layout.w
            out_frame_shape(out_fmt, oh, ow, bgr)
            on = _pitched(out, out_layout, out_fmt, 'out')
            n, h, w = _pictures(frames, layout, pix_fmt)
            if on != n:
                raise ValueError('out holds %d frames, frames holds %d' % (on, n))
            if tuple(boxes.shape) != (n, 4):
                raise ValueError('boxes of shape %s for %d frames (int32 [n, 4])' % (tuple(boxes.shape), n))
        else:
            _need_cuda(out, torch.uint8, 'out')
            n, h, w = _pictures(frames, layout, pix_fmt)
            if out_fmt == 'nv12':
                on, oh, ow = picture_size(out, 'nv12')
                out_frame_shape(out_fmt, oh, ow, bgr)
            else:
                out_frame_shape(out_fmt, 1, 1)
                assert out.shape[3] == 3
                on, oh, ow = (int(v) for v in out.shape[:3])
            assert tuple(boxes.shape) == (n, 4) and on == n

        src, window, flags = (self._h, frames, layout, pix_fmt, n, h, w), (_ptr(boxes), bw, bh, _ptr(out)), RENDER_BGR if bgr else 0
        # the entry: the first rung that holds, each one entry for everything below it (format, layout, filter, colour)
        if out_layout is not None:
            entry = 'svc_render_crops_to_layout'
            if not hasattr(self.lib, entry):
                raise _lib.SvcError('%s lacks svc_render_crops_to_layout: an out_layout needs a build that has it' % _lib.LIB_PATH)
            olay = out_layout.struct()
            args = _src_args(*src, _colour_struct(colour)) + window + (ctypes.byref(olay), _colour_struct(out_colour), oh, ow, INTERPS.index(interp), flags)
        elif colour is not None or out_colour is not None:
            entry = 'svc_render_crops_colour'
            args = _src_args(*src, _colour_struct(colour)) + window + (OUT_FMTS.index(out_fmt), _colour_struct(out_colour), oh, ow, INTERPS.index(interp), flags)
        elif interp != 'linear':
            entry, args = 'svc_render_crops_filter', _src_args(*src) + window + (OUT_FMTS.index(out_fmt), oh, ow, INTERPS.index(interp), flags)
        elif layout is not None:
            entry, args = 'svc_render_crops_layout', _src_args(*src) + window + (OUT_FMTS.index(out_fmt), oh, ow, flags)
        else:
            entry, args = RENDER_ENTRIES[pix_fmt, out_fmt], (self._h, _ptr(frames), n, h, w) + window + (oh, ow, flags)
        _lib.check(getattr(self.lib, entry)(*args, _stream()))
        return out

    def render_windows(self, frames, origins_q8, win_wh, out_hw=None, bgr=False, out=None, pix_fmt='rgb24', out_fmt='rgb24', layout=None,
                       colour=None, out_colour=None, out_layout=None):
        """render_crops(interp='linear') at sub-pixel window origins (svc_render_windows_q8; include/svc.h states the arithmetic).
        origins_q8: int32 CUDA tensor [n, 2], the top-left corner (x, y) of every frame's window in 1/256 pixel, clamped by the
        kernel into the frame; win_wh = (bw, bh), one window size for all.  out_hw None is the window size -- not a copy here but
        the window shifted by its fraction.  Origins that are multiples of 256 give the bytes of render_crops with the boxes
        (x >> 8, y >> 8, + bw, + bh).  Every other argument is render_crops's, with its checks (ValueError / TypeError before any
        device work)."""
        _side_colour(colour, pix_fmt, 'colour')
        _side_colour(out_colour, out_fmt if out_fmt in OUT_FMTS else 'nv12', 'out_colour')
        n = int(frames.shape[0])
        bw, bh = int(win_wh[0]), int(win_wh[1])
        if bw < 1 or bh < 1:
            raise ValueError('empty window %d x %d' % (bw, bh))
        oh, ow = (bh, bw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        shape = _out_shape(n, out_fmt, oh, ow, bgr, out_layout)
        if not (torch.is_tensor(origins_q8) and origins_q8.dtype == torch.int32):
            raise TypeError('origins_q8 must be a CUDA tensor of dtype torch.int32 (window origins in 1/256 pixel)')
        if tuple(origins_q8.shape) != (n, 2):
            raise ValueError('origins_q8 of shape %s for %d frames (int32 [n, 2]: x, y)' % (tuple(origins_q8.shape), n))
        _, h, w = _pictures(frames, layout, pix_fmt)
        if bw > w or bh > h:
            raise ValueError('a window of %d x %d does not fit the %d x %d picture' % (bw, bh, w, h))
        _need_cuda(origins_q8, torch.int32, 'origins_q8')
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        if out_layout is not None:
            on = _pitched(out, out_layout, out_fmt, 'out')
        else:
            _need_cuda(out, torch.uint8, 'out')
            on = int(out.shape[0])
            if tuple(out.shape) != shape:
                raise ValueError('out of shape %s, the output is %s' % (tuple(out.shape), shape))
        if on != n:
            raise ValueError('out holds %d frames, frames holds %d' % (on, n))
        if not hasattr(self.lib, 'svc_render_windows_q8'):
            raise _lib.SvcError('%s lacks svc_render_windows_q8: sub-pixel windows need a build that has it' % _lib.LIB_PATH)
        colour, out_colour = _side_colour(colour, pix_fmt, 'colour'), _side_colour(out_colour, out_fmt, 'out_colour')
        olay = (out_layout or frame_layout(out_fmt, oh, ow)).struct()       # (the packed values run the packed sinks)
        _lib.check(self.lib.svc_render_windows_q8(*_src_args(self._h, frames, layout, pix_fmt, n, h, w, _colour_struct(colour)), _ptr(origins_q8),
                                                  bw, bh, _ptr(out), ctypes.byref(olay), _colour_struct(out_colour), oh, ow,
                                                  RENDER_BGR if bgr else 0, _stream()))
        return out

    # -- saliency ------------------------------------------------------------------------
    def saliency(self, frames, out=None, threshold=0, census=None, profile=None):
        """uint8 [n,h,w,3] RGB at saliency size -> uint8 [n,h,w] maps (frame-major); `out`: write into this tensor.
        threshold > 0: the maps come out thresholded (sc_threshold fused into the network's last kernel: the bytes of
        saliency() + threshold_(), one launch less).  census (with a threshold): int32 CUDA rows [n,4] to which the pixels
        of every frame's raw map at t - 1, t, t + 1 are ADDED (svc_saliency_census_u8; the caller zeroes the rows).
        profile: int32 CUDA rows [n,h+w] into which the row and column maxima of every frame's RAW map are max-combined
        (what border_profile() gives on the un-thresholded maps, from inside the network's last kernel:
        svc_saliency_profile_u8; the caller zeroes the rows).  Maps and census are the same bytes with and without it."""
        _need_cuda(frames, torch.uint8, 'frames')
        n, h, w, c = frames.shape
        assert c == 3
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.uint8, device=frames.device)
        else:
            _need_cuda(out, torch.uint8, 'out')
            assert tuple(out.shape) == (n, h, w)
        if census is not None:
            _need_cuda(census, torch.int32, 'census')
            assert threshold and tuple(census.shape) == (n, 4)
        if profile is not None:
            _need_cuda(profile, torch.int32, 'profile')
            assert tuple(profile.shape) == (n, h + w)
            _lib.check(self.lib.svc_saliency_profile_u8(self._h, _ptr(frames), n, h, w, _ptr(out), int(threshold),
                                                        _ptr(census) if census is not None else None, _ptr(profile), _stream()))
        elif census is not None:
            _lib.check(self.lib.svc_saliency_census_u8(self._h, _ptr(frames), n, h, w, _ptr(out), int(threshold), _ptr(census), _stream()))
        elif threshold:
            _lib.check(self.lib.svc_saliency_thresholded_u8(self._h, _ptr(frames), n, h, w, _ptr(out), int(threshold), _stream()))
        else:
            _lib.check(self.lib.svc_saliency_u8(self._h, _ptr(frames), n, h, w, _ptr(out), _stream()))
        return out

    def border_profile(self, maps, out=None):
        """RAW uint8 [n,h,w] maps -> int32 [n,h+w] rows: [i,:h] the maxima of map i's rows (max over x), [i,h:] of its columns
        (max over y): the device half of sc_border_detection (svc_border_profile_u8).  `out`: rows to max-combine into
        (not overwritten); without it a zeroed tensor is made.  A video's profile is out.amax(0)."""
        _need_cuda(maps, torch.uint8, 'maps')
        n, h, w = maps.shape
        if out is None:
            out = torch.zeros((n, h + w), dtype=torch.int32, device=maps.device)
        else:
            _need_cuda(out, torch.int32, 'out')
            assert tuple(out.shape) == (n, h + w)
        _lib.check(self.lib.svc_border_profile_u8(self._h, _ptr(maps), n, h, w, _ptr(out), _stream()))
        return out

    def tap(self, which, frame, shape):
        out = np.empty(int(np.prod(shape)), np.float32)
        _lib.check(self.lib.svc_debug_tap(self._h, which, frame, out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out.reshape(shape)

    def run_node(self, node, n, height, width, in0, in1=None, out_shape=None):
        """Test door (svc_debug_run_node): one node of the network on the caller's host arrays -- fp32 NHWC of n frames (uint8
        frames for NODE_FRONT) -- for saliency maps of height x width.  -> fp32 [n, *out_shape] (out_shape: the per-frame shape
        of the node's output buffer; include/svc.h lists them -- (2, height, width) for NODE_MAP / NODE_MAP_PROFILE: the
        pre-softmax map and the uint8 map's values as floats).  What the node did not write comes back as NaN."""
        vp = ctypes.c_void_p
        in0 = np.ascontiguousarray(in0, np.uint8 if node == NODE_FRONT else np.float32)
        in1 = None if in1 is None else np.ascontiguousarray(in1, np.float32)
        out = np.empty((n,) + tuple(int(v) for v in out_shape), np.float32)
        per = _lib.check(self.lib.svc_debug_run_node(self._h, int(node), int(n), int(height), int(width), in0.ctypes.data_as(vp),
                                                     None if in1 is None else in1.ctypes.data_as(vp), out.ctypes.data_as(vp), out.size))
        if per * n != out.size:
            raise ValueError('node %d writes %d floats per frame, not %s' % (node, per, out.shape[1:]))
        return out

    # -- tail ----------------------------------------------------------------------------
    def threshold_(self, maps, t):
        _need_cuda(maps, torch.uint8, 'maps')
        _lib.check(self.lib.svc_threshold_u8(self._h, _ptr(maps), maps.numel(), int(t), _stream()))
        return maps

    def cluster_center_(self, maps, blend_flags, CP, want_stats=False):
        """In place on thresholded uint8 [n,h,w] maps.  blend_flags: host sequence of n flags (or None): True / BLEND_NEXT =
        blend map i into map i+1 once it is final; MAP_HELD = not processed by this call (already final, or left for a
        later one), so a blend chain can be carried over between calls.  -> xy float64 [n,2] (NaN = None; unspecified for
        held maps) [, stats int32 [n,4]]."""
        _need_cuda(maps, torch.uint8, 'maps')
        n, h, w = maps.shape
        p = _lib.make_params(CP)
        xy = torch.empty((n, 2), dtype=torch.float64, device=maps.device)
        stats = torch.zeros((n, 4), dtype=torch.int32, device=maps.device) if want_stats else None
        flags = None
        if blend_flags is not None:
            flags = np.ascontiguousarray(np.asarray(blend_flags, np.uint8))
            assert flags.shape == (n,)
        _lib.check(self.lib.svc_cluster_center(
            self._h, _ptr(maps), n, h, w, flags.ctypes.data_as(ctypes.c_void_p) if flags is not None else None,
            ctypes.byref(p), _ptr(xy), _ptr(stats) if want_stats else None, _stream()))
        return (xy, stats) if want_stats else xy

    def tail_plan(self, h, w, CP):
        """Test door (svc_debug_tail_plan): what cluster_center_ plans for maps of h x w with CP on this engine, and the thresholds
        by which the tail's kernels choose a form per map, as a dict of TAIL_PLAN_WORDS ('h', 'w': the shape the tail clusters
        on, after resize_factor).  Host arithmetic of the library: nothing is launched."""
        if not hasattr(self.lib, 'svc_debug_tail_plan'):
            raise _lib.SvcError('%s lacks svc_debug_tail_plan: the plan door of the tail needs a build that has it' % _lib.LIB_PATH)
        p = _lib.make_params(CP)
        out = (ctypes.c_int32 * len(TAIL_PLAN_WORDS))()
        n = _lib.check(self.lib.svc_debug_tail_plan(self._h, int(h), int(w), ctypes.byref(p), ctypes.cast(out, ctypes.c_void_p), len(TAIL_PLAN_WORDS)))
        if n != len(TAIL_PLAN_WORDS):
            raise _lib.SvcError('svc_debug_tail_plan reports %d words, this binding knows %d' % (n, len(TAIL_PLAN_WORDS)))
        return dict(zip(TAIL_PLAN_WORDS, (int(v) for v in out)))

    # -- measurement door (bench.py) -------------------------------------------------------
    KERNEL_CLASSES = ('resize', 'lanczos', 'stem', 'pw', 'dw', 'resample', 'smooth', 'threshold', 'compact',
                      'core', 'prim', 'finish')
    PROFILE_CLASSES = KERNEL_CLASSES + ('render', 'border')   # 'render' (svc_render_crops_u8) is behind the saliency-to-crop path;
    #                                                        'border' = svc_border_profile_u8 (the fused form counts under 'smooth')

    def profile_enable(self, kernel_class):
        """kernel_class: name from PROFILE_CLASSES, or None to switch event recording off."""
        k = -1 if kernel_class is None else self.PROFILE_CLASSES.index(kernel_class)
        _lib.check(self.lib.svc_profile_enable(self._h, k))

    def profile_read(self):
        """-> (total_ms, launches) of the profiled class since the last read; synchronises."""
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        _lib.check(self.lib.svc_profile_read(self._h, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def profile_read_raw(self):
        """-> (raw_total_ms, empty_pair_ms, launches): the ingredients of profile_read's corrected sum."""
        raw, pair, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _lib.check(self.lib.svc_profile_read_raw(self._h, ctypes.byref(raw), ctypes.byref(pair), ctypes.byref(cnt)))
        return raw.value, pair.value, cnt.value

    def front_fused(self):
        """True when the last saliency call ran LANCZOS + features.0 + features.1 as the one kernel k_front."""
        return bool(self.lib.svc_front_fused(self._h))

    def threshold_census(self, reset=False):
        """-> dict(maps, below, at, above, pixels_per_grey_level): pixels of the un-thresholded maps at t - 1 / t / t + 1 over
        the maps this engine produced through saliency(threshold=t) since the last reset (svc_threshold_census: the regime
        diagnostic of the threshold; synchronises)."""
        out = (ctypes.c_uint64 * 4)()
        _lib.check(self.lib.svc_threshold_census(self._h, ctypes.cast(out, ctypes.c_void_p), 1 if reset else 0))
        maps, lo, at, hi = (int(v) for v in out)
        return dict(maps=maps, below=lo, at=at, above=hi, pixels_per_grey_level=((lo + at + hi) / (3.0 * maps) if maps else None))

    def matrix_pipe(self):
        """'f32' (fp32 MFMA) or 'bf16x6' (split-bf16 operands, six plane pairs on the bf16 MFMA): what the handle's 1x1
        convolutions run on (svc_matrix_pipe; environment SVC_MX when the engine is created)."""
        return 'bf16x6' if self.lib.svc_matrix_pipe(self._h) == 6 else 'f32'

    def argsort_u32(self, keys):
        """Test door: the device's emulation of numpy's default argsort on uint32 keys -> int32 order."""
        keys = np.ascontiguousarray(keys, np.uint32)
        out = np.empty(keys.size, np.int32)
        vp = ctypes.c_void_p
        _lib.check(self.lib.svc_debug_argsort_u32(self._h, keys.ctypes.data_as(vp), keys.size, out.ctypes.data_as(vp)))
        return out

    def cluster_state(self, frame, cap):
        pts = np.zeros(cap, np.uint32)
        core = np.zeros(cap, np.uint32)
        mst = np.zeros((cap, 3), np.uint32)
        labels = np.zeros(cap, np.int32)
        hdr = np.zeros(HDR_WORDS, np.int32)
        vp = ctypes.c_void_p
        n = _lib.check(self.lib.svc_debug_cluster_state(self._h, frame, cap, pts.ctypes.data_as(vp),
                                                         core.ctypes.data_as(vp), mst.ctypes.data_as(vp),
                                                         labels.ctypes.data_as(vp), hdr.ctypes.data_as(vp)))
        m = min(n, cap)
        return dict(n=n, pts=pts[:m], core=core[:m], mst=mst[:max(m - 1, 0)], labels=labels[:m], hdr=hdr)


TAIL_KNOBS = ('SVC_PRIM_LVL', 'SVC_TREE_PAR', 'SVC_TAIL_MERGE')       # read by svc_create


def tail_engine(reference, state_dict=None, seed=0):
    """An Engine whose tail form does not depend on the caller's environment.  reference=True: the one-node-per-step Prim
    (k_prim_ref), the serial hierarchy (k_tree) and one kernel per stage -- the second device reference of the tests, itself
    checked against the oracle; False: the default form (the three knobs unset).  The environment is restored."""
    import os
    saved = {k: os.environ.pop(k, None) for k in TAIL_KNOBS}
    try:
        if reference:
            os.environ.update({k: '0' for k in TAIL_KNOBS})
        return Engine(state_dict, seed=seed)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def iou_boxes(a, b):
    """IoU (inclusive +1 convention) of int32 box arrays [M,4] on the GPU -> float64 numpy [M].
    Accepts numpy arrays or CUDA tensors."""
    if not torch.cuda.is_available():
        raise _lib.SvcError('no GPU visible: svc_iou_i32 runs on the MI355X only')
    lib = _lib.load()
    ta = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    tb = b if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b, np.int32)).cuda()
    _need_cuda(ta, torch.int32, 'a')
    _need_cuda(tb, torch.int32, 'b')
    assert ta.shape == tb.shape and ta.shape[-1] == 4
    m = ta.shape[0]
    out = torch.empty(m, dtype=torch.float64, device=ta.device)
    _lib.check(lib.svc_iou_i32(_ptr(ta), _ptr(tb), m, _ptr(out), _stream()))
    return out.cpu().numpy()


def focus_jumps(maps, xy, min_d):
    """The jump statistics of the focus stability from maps that stay on the device (svc_focus_jumps_u8, include/svc.h): maps =
    the FILTERED maps, a contiguous CUDA uint8 [n, h, w] tensor; xy = the centres before the hold, a CUDA float64 [n, 2] tensor on
    the maps' device, or a NumPy array / list that is uploaded there.  -> CUDA int32 [n, 2]: row i >= 1 = (sum, count) of map i's
    values along the move xy[i-1] -> xy[i]; count 0 = no statistic (jump 255), count -1 = a centre outside the entry's domain
    (not finite, or beyond 65 536); row 0 = (0, 0).  Runs on the maps' device and the current stream; no handle, no scratch."""
    lib = _lib.load()
    if not hasattr(lib, 'svc_focus_jumps_u8'):
        raise _lib.SvcError('%s lacks svc_focus_jumps_u8: the device focus stability needs a build that has it' % _lib.LIB_PATH)
    _need_cuda(maps, torch.uint8, 'maps')
    if maps.dim() != 3:
        raise ValueError('maps must be [n, h, w], not %s' % (tuple(maps.shape),))
    n, h, w = (int(v) for v in maps.shape)
    if not torch.is_tensor(xy):
        xy = torch.from_numpy(np.ascontiguousarray(xy, np.float64).reshape(-1, 2)).to(maps.device)
    _need_cuda(xy, torch.float64, 'xy')
    if tuple(xy.shape) != (n, 2) or xy.device != maps.device:
        raise ValueError('xy must be [%d, 2] on %s, not %s on %s' % (n, maps.device, tuple(xy.shape), xy.device))
    with torch.cuda.device(maps.device):
        out = torch.empty((n, 2), dtype=torch.int32, device=maps.device)
        _lib.check(lib.svc_focus_jumps_u8(_ptr(maps), n, h, w, _ptr(xy), float(min_d), _ptr(out), _stream()))
    return out


def _demo_i32(v, shape, name, dev):
    """A host array / list -> contiguous int32 CUDA tensor of `shape` on dev (a tensor is checked, not copied)."""
    if not torch.is_tensor(v):
        a = np.ascontiguousarray(v, np.int32)
        if a.shape != shape:
            raise ValueError('%s must be int32 %s, not %s' % (name, list(shape), a.shape))
        return torch.from_numpy(a).to(dev)
    if v.dtype != torch.int32 or tuple(v.shape) != shape or not v.is_contiguous() or v.device != dev:
        raise ValueError('%s must be a contiguous int32 %s tensor on %s, not %s %s on %s' % (name, list(shape), dev, v.dtype, tuple(v.shape), v.device))
    return v


def demo_frames(small, raw, filt, map_of, marks, first, atlas, bgr=False, out=None):
    """The five-panel demo frames (svc_demo_frames_u8; include/svc.h states the panels and the marks): small = the frames at the
    process size, a contiguous CUDA uint8 [n, ph, pw, 3] RGB tensor (Engine.resize_frames makes it); raw, filt = the raw and the
    filtered maps, contiguous CUDA uint8 [n_maps, ph, pw] each; map_of int32 [n] = the map of every frame (outside [0, n_maps): an
    all-zero map); marks int32 [k, 8] and first int32 [n + 1] = the marks of frame f are rows first[f] .. first[f + 1] (render.demo_marks
    makes the three); atlas = the uint8 coverage sprites the TEXT marks point into (render.demo_atlas), or None.  map_of, marks,
    first and atlas are CUDA tensors on small's device, or host arrays that are uploaded there.  bgr: every pixel stored (b, g, r).
    -> out, a contiguous CUDA uint8 [n, ph, 5 * pw, 3] tensor (allocated unless given).  Every shape, dtype and device is checked
    first: ValueError before any device work.  Runs on small's device and the current stream; no handle, no scratch."""
    lib = _lib.load()
    if not hasattr(lib, 'svc_demo_frames_u8'):
        raise _lib.SvcError('%s lacks svc_demo_frames_u8: the demo frames need a build that has it' % _lib.LIB_PATH)

    def u8(t, name, dims):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == dims):
            raise ValueError('%s must be a contiguous CUDA uint8 tensor of %d dimensions' % (name, dims))
    u8(small, 'small', 4)
    n, ph, pw, ch = (int(v) for v in small.shape)
    dev = small.device
    if ch != 3 or ph < 1 or pw < 1:
        raise ValueError('small must be [n, ph, pw, 3] with ph, pw >= 1, not %s' % (tuple(small.shape),))
    u8(raw, 'raw', 3)
    u8(filt, 'filt', 3)
    n_maps = int(raw.shape[0])
    for t, name in ((raw, 'raw'), (filt, 'filt')):
        if tuple(t.shape) != (n_maps, ph, pw) or t.device != dev:
            raise ValueError('%s must be [%d, %d, %d] on %s, not %s on %s' % (name, n_maps, ph, pw, dev, tuple(t.shape), t.device))
    k = int(marks.shape[0]) if hasattr(marks, 'shape') and len(marks.shape) == 2 else len(marks)
    map_of = _demo_i32(map_of, (n,), 'map_of', dev)
    marks = _demo_i32(marks if k else np.zeros((0, _lib.MARK_WORDS), np.int32), (k, _lib.MARK_WORDS), 'marks', dev)
    first = _demo_i32(first, (n + 1,), 'first', dev)
    if atlas is not None:
        if not torch.is_tensor(atlas):
            a = np.ascontiguousarray(atlas)
            if a.dtype != np.uint8 or a.ndim != 1:
                raise ValueError('atlas must be uint8 [bytes], not %s %s' % (a.dtype, a.shape))
            atlas = torch.from_numpy(a).to(dev)
        u8(atlas, 'atlas', 1)
        if atlas.device != dev:
            raise ValueError('atlas must be on %s, not %s' % (dev, atlas.device))
    shape = (n, ph, 5 * pw, 3)
    if out is not None:
        u8(out, 'out', 4)
        if tuple(out.shape) != shape or out.device != dev:
            raise ValueError('out must be %s on %s, not %s on %s' % (list(shape), dev, tuple(out.shape), out.device))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        n_atlas = int(atlas.numel()) if atlas is not None else 0
        _lib.check(lib.svc_demo_frames_u8(_ptr(small), n, ph, pw, _ptr(raw) if n_maps else None, _ptr(filt) if n_maps else None, n_maps,
                                          _ptr(map_of), _ptr(marks) if k else None, k, _ptr(first), _ptr(atlas) if n_atlas else None, n_atlas,
                                          _ptr(out), RENDER_BGR if bgr else 0, _stream()))
    return out
