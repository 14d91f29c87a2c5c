"""NV12 colour on the host (no GPU): the table of include/svc.h against the rule it is derived by, the arithmetic's ranges over
every YUV and every RGB triple, the header against the binding, and the refusals of the Python doors and of the two C entries
before any device work.  colour_ref states the formulas (int64 intermediates)."""
import ctypes
import os
import re

import numpy as np
import pytest

import colour_ref as C
import nv12_out_ref
import nv12_ref
from retargetvid_amd import _lib, ingest, ops, render, smartVidCrop as S
from retargetvid_amd.frames import FrameSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 36, 64


def _header():
    return open(os.path.join(ROOT, 'include', 'svc.h')).read()


# ---------------------------------------------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('matrix,rng', C.NEW_VARIANTS)
def test_the_derived_rows_follow_the_rule(matrix, rng):
    """Kr, Kb as exact fractions, every coefficient times 2^20 rounded half away from zero, YG / UG / VG as the remainders."""
    assert C.derive(matrix, rng) == C.TABLE[matrix, rng]


def test_bt601_limited_is_the_row_it_always_was():
    dec, enc = C.TABLE[C.DEFAULT]
    assert dec == (16, nv12_ref.CY, nv12_ref.CVR, nv12_ref.CVG, nv12_ref.CUG, nv12_ref.CUB)
    assert enc == nv12_out_ref.Y_COEF + nv12_out_ref.U_COEF + nv12_out_ref.V_COEF
    assert C.derive(*C.DEFAULT) != C.TABLE[C.DEFAULT]               # OpenCV's three-decimal coefficients, not the rule's
    rng = np.random.RandomState(0)
    nv = rng.randint(0, 256, (2, 54, 64)).astype(np.uint8)
    rgb = rng.randint(0, 256, (2, 36, 64, 3)).astype(np.uint8)
    for colour in (None, C.DEFAULT, dict(matrix='bt601'), dict()):
        assert np.array_equal(C.nv12_to_rgb(nv, 36, 64, colour), nv12_ref.nv12_to_rgb(nv, 36, 64))
        assert np.array_equal(C.rgb_to_nv12(rgb, colour), nv12_out_ref.rgb_to_nv12_fixed(rgb))


def test_remainders_make_white_and_grey_exact():
    for (matrix, rng), (dec, enc) in C.TABLE.items():
        if (matrix, rng) == C.DEFAULT:
            continue
        assert sum(enc[:3]) == C._round((C.Fraction(219, 255) if rng == 'limited' else C.Fraction(1)))
        assert sum(enc[3:6]) == 0 and sum(enc[6:]) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# every triple, both directions
# ---------------------------------------------------------------------------------------------------------------------------
def _py_encode(variant, r, g, b):
    """One flat colour through the encode formula in Python integers, unclamped -> (Y, U, V)."""
    dec, (yr, yg, yb, ur, ug, ub, vr, vg, vb) = C.TABLE[variant]
    y = (yr * r + yg * g + yb * b + (dec[0] << 20) + (1 << 19)) >> 20
    u = (4 * (ur * r + ug * g + ub * b) + (128 << 22) + (1 << 21)) >> 22
    v = (4 * (vr * r + vg * g + vb * b) + (128 << 22) + (1 << 21)) >> 22
    return y, u, v


# black, white, pure red, pure blue -> (Y, U, V) before the clamp, read off the formula by hand
LANDMARKS = {
    ('bt601', 'limited'): ((16, 128, 128), (235, 128, 128), (82, 90, 240), (41, 240, 110)),
    ('bt601', 'full'): ((0, 128, 128), (255, 128, 128), (76, 85, 256), (29, 256, 107)),
    ('bt709', 'limited'): ((16, 128, 128), (235, 128, 128), (63, 102, 240), (32, 240, 118)),
    ('bt709', 'full'): ((0, 128, 128), (255, 128, 128), (54, 99, 256), (18, 256, 116)),
}


@pytest.mark.parametrize('variant', C.VARIANTS)
def test_landmark_colours(variant):
    colours = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255))
    assert tuple(_py_encode(variant, *c) for c in colours) == LANDMARKS[variant]
    flat = np.array(colours, np.uint8)[:, None, None, :].repeat(2, 1).repeat(2, 2)       # four 2 x 2 crops
    got = C.rgb_to_nv12(flat, variant)
    assert [(int(f[0, 0]), int(f[2, 0]), int(f[2, 1])) for f in got] == [tuple(min(v, 255) for v in t) for t in LANDMARKS[variant]]
    # and back: black and white are exact in every variant
    back = C.nv12_to_rgb(got, 2, 2, variant)
    assert back[0].max() == 0 and back[1].min() == 255


@pytest.mark.parametrize('variant', C.VARIANTS)
def test_every_triple_stays_in_range(variant):
    """All 2^24 (Y, U, V) and all 2^24 (r, g, b): the bounds the kernels rely on (24-bit factors, int32 sums), where the
    outputs land before the clamp, and the round trip of a flat colour."""
    dec, enc = C.TABLE[variant]
    limited = variant[1] == 'limited'
    assert all(abs(c) < 1 << 23 for c in dec[1:] + enc)                 # __mul24 is exact
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')   # the two fast coordinates of a 65536-triple slab
    dec_hi = 0
    enc_lo, enc_hi = 1 << 62, 0
    y_rng, u_rng, v_rng = [255, 0], [1 << 30, 0], [1 << 30, 0]
    worst = 0
    for k in range(256):
        raw = C.yuv_to_rgb_raw(np.full_like(a, k), a, b, variant)       # Y = k, every (U, V)
        dec_hi = max(dec_hi, int(np.abs(raw).max()))
        # r = k, every (g, b): a flat colour, whose block sums are 4 r, 4 g, 4 b
        y = C.luma_raw(k, a, b, variant)
        u, v = C.chroma_raw(4 * k, 4 * a, 4 * b, variant)
        enc_lo = min(enc_lo, int(y.min()), int(u.min()), int(v.min()))
        enc_hi = max(enc_hi, int(y.max()), int(u.max()), int(v.max()))
        for rng_, val in ((y_rng, y >> 20), (u_rng, u >> 22), (v_rng, v >> 22)):
            rng_[0], rng_[1] = min(rng_[0], int(val.min())), max(rng_[1], int(val.max()))
        back = C.yuv_to_rgb(np.clip(y >> 20, 0, 255), np.clip(u >> 22, 0, 255), np.clip(v >> 22, 0, 255), variant).astype(np.int64)
        worst = max(worst, int(np.abs(back - np.stack([np.full_like(a, k), a, b], -1)).max()))
    assert dec_hi <= 5.8e8
    assert 5.2e5 <= enc_lo and enc_hi <= 1.074e9 and enc_hi < 2 ** 31
    # (the chroma sums are linear in the block sums: over every block, not only the flat ones, the extremes are at corners)
    off = (128 << 22) + (1 << 21)
    for co in (enc[3:6], enc[6:]):
        assert off + 1020 * sum(c for c in co if c < 0) >= 5.2e5 and off + 1020 * sum(c for c in co if c > 0) <= 1.074e9
    if limited:
        assert (y_rng, u_rng, v_rng) == ([16, 235], [16, 240], [16, 240])           # nothing to clamp
    else:
        assert (y_rng, u_rng, v_rng) == ([0, 255], [1, 256], [1, 256])              # 256: pure blue (U), pure red (V)
    assert worst <= (2 if limited else 1)


# ---------------------------------------------------------------------------------------------------------------------------
# header and binding
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_binding_agree():
    hdr = _header()
    val = lambda name: int(re.search(r'#define %s\s+(\d+)' % name, hdr).group(1))
    assert (val('SVC_MATRIX_BT601'), val('SVC_MATRIX_BT709')) == (_lib.MATRIX_BT601, _lib.MATRIX_BT709) \
        == (ops.MATRICES.index('bt601'), ops.MATRICES.index('bt709')) == (0, 1)
    assert (val('SVC_RANGE_LIMITED'), val('SVC_RANGE_FULL')) == (_lib.RANGE_LIMITED, _lib.RANGE_FULL) \
        == (ops.RANGES.index('limited'), ops.RANGES.index('full')) == (0, 1)
    body = re.search(r'typedef struct SvcColour \{(.*?)\} SvcColour;', hdr, flags=re.S).group(1)
    fields = re.findall(r'\b(u?int32_t)\s+(\w+);', body)
    ctype = dict(uint32_t=ctypes.c_uint32, int32_t=ctypes.c_int32)
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.SvcColour._fields_)
    assert ctypes.sizeof(_lib.SvcColour) == 16
    assert ops.MATRICES == C.MATRICES and ops.RANGES == C.RANGES and ops.DEFAULT_COLOUR == C.DEFAULT
    for name in ('svc_resize_frames_colour', 'svc_render_crops_colour'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    s = ops._colour_struct(('bt709', 'full'))._obj
    assert (s.struct_size, s.matrix, s.range, s.reserved) == (16, 1, 1, 0) and ops._colour_struct(None) is None


def test_the_header_states_the_table():
    text = re.search(r'/\* The colour of NV12 frames.*?\*/', _header(), flags=re.S).group(0)
    numbers = set(int(v) for v in re.findall(r'(?<![\w.])-?\d+(?![\w.])', text))
    for variant, (dec, enc) in C.TABLE.items():
        row = re.search(r'\* +%s +%s +(.*)' % variant, text).group(1)
        assert [int(v) for v in re.findall(r'-?\d+', row)] == list(dec + enc), variant
        assert set(dec + enc) <= numbers


# ---------------------------------------------------------------------------------------------------------------------------
# the Python doors
# ---------------------------------------------------------------------------------------------------------------------------
def _nv12_dict(n=4, **extra):
    return dict(dict(frames=np.zeros((n, H * 3 // 2, W), np.uint8), fr=25.0, frame_count=n, w=W, h=H, pix_fmt='nv12', trans_inds=[0, n]),
                **extra)


SPELLINGS = {
    ('bt601', 'limited'): (None, {}, dict(matrix='bt601'), dict(range='limited'), dict(matrix=None, range=None), ('bt601', 'limited'),
                           ['BT601', 'TV'], dict(matrix='smpte170m', range='mpeg'), dict(matrix='bt470bg')),
    ('bt601', 'full'): (dict(range='full'), dict(matrix='bt601', range='full'), ('bt601', 'full'), dict(matrix='BT601', range='PC'),
                        dict(matrix='bt470bg', range='jpeg')),
    ('bt709', 'limited'): (dict(matrix='bt709'), dict(matrix='bt709', range='limited'), ('bt709', 'limited'), dict(matrix='BT709', range='tv'),
                           dict(matrix='bt709', range=None)),
    ('bt709', 'full'): (dict(matrix='bt709', range='full'), ('bt709', 'full'), ['bt709', 'full'], dict(matrix='Bt709', range='Jpeg'),
                        dict(matrix='bt709', range='pc')),
}


@pytest.mark.parametrize('variant', C.VARIANTS)
def test_every_spelling_is_accepted(variant):
    for spec in SPELLINGS[variant]:
        assert ops.frame_colour(spec) == variant, spec
        assert FrameSource.of(_nv12_dict(colour=spec)).colour == variant
        assert FrameSource.of(np.zeros((2, H * 3 // 2, W), np.uint8), 'nv12', None, spec).colour == variant
    assert ops.frame_colour(variant) == variant


@pytest.mark.parametrize('spec,text', [
    (dict(matrix='bt2020'), "unknown colour matrix 'bt2020'"),
    (dict(matrix='bt709', range='wide'), "unknown colour range 'wide'"),
    (('bt709', 'limited', 0), 'a colour is dict'),
    ('bt709', 'a colour is dict'),
    (dict(matrix='bt709', rnage='full'), "unknown colour key 'rnage'"),
    (dict(matrix=1), 'unknown colour matrix 1'),
])
def test_an_unknown_colour_is_refused(spec, text):
    VD = dict(fc=0, bbs_np=np.zeros((0, 4), np.int64))
    for door in (ops.frame_colour, lambda s: FrameSource.of(_nv12_dict(colour=s)), lambda s: S.video_pix_fmt(_nv12_dict(colour=s)),
                 lambda s: S.plan_video(_nv12_dict(colour=s), S.sc_init_crop_params()),
                 lambda s: render.render_video(_nv12_dict(), VD, out_fmt='nv12', out_colour=s),
                 lambda s: S.smart_vid_crop(_nv12_dict(), save_vid=False, out_pix_fmt='nv12', out_colour=s, engine=object())):
        with pytest.raises(ValueError) as e:
            door(spec)
        assert text in str(e.value)


def test_rgb_has_no_colour():
    rgb = dict(frames=np.zeros((4, H, W, 3), np.uint8), fr=25.0, frame_count=4, w=W, h=H, trans_inds=[0, 4])
    assert FrameSource.of(rgb).colour is None and FrameSource.of(_nv12_dict()).colour == ('bt601', 'limited')
    VD = dict(fc=0, bbs_np=np.zeros((0, 4), np.int64))
    for colour in (dict(matrix='bt709'), dict(), ('bt601', 'limited')):           # the default spelled out is a colour too
        for door in (lambda c: FrameSource.of(dict(rgb, colour=c)), lambda c: FrameSource.of(rgb['frames'], 'rgb24', None, c),
                     lambda c: S.plan_video(dict(rgb, colour=c), S.sc_init_crop_params()),
                     lambda c: render.render_video(dict(rgb, colour=c), VD),
                     lambda c: render.render_video(rgb, VD, out_colour=c),                        # out_fmt='rgb24'
                     lambda c: render.render_video(_nv12_dict(), VD, out_fmt='rgb24', out_colour=c),
                     lambda c: S.smart_vid_crop(rgb, save_vid=False, out_colour=c, engine=object()),
                     lambda c: S.smart_vid_crop(_nv12_dict(), save_vid=False, out_pix_fmt='rgb24', out_colour=c, engine=object())):
            with pytest.raises(ValueError) as e:
                door(colour)
            assert 'nv12' in str(e.value)
    assert FrameSource.of(dict(rgb, colour=None)).colour is None                  # None is no colour
    # an NV12 render of frames that hold no picture: every door up to the device accepts a colour, in and out
    assert render.render_video(_nv12_dict(colour=dict(matrix='bt709')), VD, out_size=(2, 2), out_fmt='nv12', out_colour=('bt601', 'full')).shape == (0, 3, 2)
    assert render.render_video(rgb, VD, out_size=(2, 2), out_fmt='nv12', out_colour=('bt709', 'full')).shape == (0, 3, 2)


def test_the_cache_key_carries_a_colour_that_is_not_the_default():
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    eng = type('E', (), dict(weights_id=1))()
    plain = _nv12_dict()
    assert FrameSource.of(plain).key() == dict(pix_fmt='nv12')                    # what it is without this feature
    for spec in SPELLINGS[C.DEFAULT]:
        assert FrameSource.of(_nv12_dict(colour=spec)).key() == dict(pix_fmt='nv12')
        assert S.feature_cache_key(_nv12_dict(colour=spec), CP, eng) == S.feature_cache_key(plain, CP, eng)
    keys = [S.feature_cache_key(_nv12_dict(colour=v), CP, eng) for v in C.VARIANTS]
    assert all(keys[i] != keys[j] for i in range(4) for j in range(i))
    assert 'colour' not in keys[0] and keys[3]['colour'] == ('bt709', 'full')
    assert FrameSource.of(_nv12_dict(colour=dict(matrix='bt709'))).key() == dict(pix_fmt='nv12', colour=('bt709', 'limited'))
    lay = dict(pitch=128, chroma_offset=128 * 48)
    pitched = dict(_nv12_dict(), frames=np.zeros((4, 128 * 72), np.uint8), layout=lay)
    assert FrameSource.of(dict(pitched, colour=('bt709', 'full'))).key() == dict(FrameSource.of(pitched).key(), colour=('bt709', 'full'))
    import pickle
    assert pickle.loads(pickle.dumps(keys[3])) == keys[3]


def test_the_raw_writer_takes_a_colour_and_ignores_it(tmp_path):
    w = ingest.write_frames_raw(str(tmp_path / 'a.nv12'), 25.0, (4, 2), pix_fmt='nv12', colour=dict(matrix='bt709', range='full'))
    w.write(np.arange(12, dtype=np.uint8).reshape(3, 4))
    w.release()
    assert open(str(tmp_path / 'a.nv12'), 'rb').read() == bytes(range(12))


# ---------------------------------------------------------------------------------------------------------------------------
# the C entries, before any device work
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_colour_entries_refuse_without_a_device():
    lib = _lib.load()
    nv = ops.frame_layout('nv12', H, W).struct()
    rgb = ops.frame_layout('rgb24', H, W).struct()
    col = lambda m=1, r=1, size=16, res=0: _lib.SvcColour(size, m, r, res)
    ref = lambda c: None if c is None else ctypes.byref(c)

    def resize(lay, c):
        rc = lib.svc_resize_frames_colour(None, None, ctypes.byref(lay), ref(c), 0, H, W, None, 14, 25, None)
        return rc, lib.svc_last_error().decode()

    def render(lay, cin, out_fmt, cout, filt=0):
        rc = lib.svc_render_crops_colour(None, None, ctypes.byref(lay), ref(cin), 0, H, W, None, 16, 16, None, out_fmt, ref(cout), 16, 16,
                                         filt, 0, None)
        return rc, lib.svc_last_error().decode()
    # no handle: refused as the layout entries refuse it, with or without colours, by the entry's own name
    for c in (None, col(), col(0, 0)):
        rc, msg = resize(nv, c)
        assert rc == -1 and msg.startswith('svc_resize_frames_colour: invalid argument')
        for filt in (0, 1):
            rc, msg = render(nv, c, 1, c, filt)
            assert rc == -1 and msg.startswith('svc_render_crops_colour: invalid argument')
    rc, msg = resize(rgb, None)
    assert rc == -1 and msg.startswith('svc_resize_frames_colour: invalid argument')
    # a stale struct
    for size in (12, 20):
        rc, msg = resize(nv, col(size=size))
        assert rc == -1 and 'colour: SvcColour.struct_size is %d' % size in msg and '16' in msg
        rc, msg = render(nv, col(size=size), 1, None)
        assert rc == -1 and 'in_colour: SvcColour.struct_size is %d' % size in msg
        rc, msg = render(nv, None, 1, col(size=size))
        assert rc == -1 and 'out_colour: SvcColour.struct_size is %d' % size in msg
    # unknown values
    for bad, text in ((col(m=2), 'unknown matrix 2'), (col(m=-1), 'unknown matrix -1'), (col(r=2), 'unknown range 2'),
                      (col(r=-1), 'unknown range -1'), (col(res=1), 'reserved is 1')):
        rc, msg = resize(nv, bad)
        assert rc == -1 and 'svc_resize_frames_colour: colour: ' + text in msg
        rc, msg = render(nv, bad, 1, None)
        assert rc == -1 and 'svc_render_crops_colour: in_colour: ' + text in msg
        rc, msg = render(rgb, None, 1, bad, 1)
        assert rc == -1 and 'svc_render_crops_colour: out_colour: ' + text in msg
    # a colour for an RGB side, the default one included
    for c in (col(), col(0, 0)):
        rc, msg = resize(rgb, c)
        assert rc == -1 and 'colour is given but that side is rgb24' in msg
        rc, msg = render(rgb, c, 1, None)
        assert rc == -1 and 'in_colour is given but that side is rgb24' in msg
        rc, msg = render(nv, None, 0, c)
        assert rc == -1 and 'out_colour is given but that side is rgb24' in msg
    # the rules of the entries they extend come first and keep their words
    rc, msg = resize(_lib.SvcFrameLayout(32, 1, 3456, 64, 2304, 64), col())
    assert rc == -1 and 'SvcFrameLayout.struct_size is 32' in msg
    rc, msg = render(nv, col(), 2, col())
    assert rc == -1 and 'unknown out_fmt 2' in msg
    rc, msg = render(nv, col(), 1, col(), 2)
    assert rc == -1 and 'svc_render_crops_colour: unknown filter 2' in msg
    # the entries they extend keep their names
    rc = lib.svc_render_crops_filter(None, None, ctypes.byref(nv), 0, H, W, None, 16, 16, None, 1, 16, 16, 0, 0, None)
    assert rc == -1 and lib.svc_last_error().decode().startswith('svc_render_crops_layout: invalid argument')
    rc = lib.svc_render_crops_filter(None, None, ctypes.byref(nv), 0, H, W, None, 16, 16, None, 1, 16, 16, 1, 0, None)
    assert rc == -1 and lib.svc_last_error().decode().startswith('svc_render_crops_filter: invalid argument')
