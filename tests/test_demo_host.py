"""The demo video without a GPU: the entry's place in the header and the binding, its argument checks, the mark lists of
render.demo_marks against hand-worked ones, the label atlas, and the demo_fn door of smart_vid_crop before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

from retargetvid_amd import _lib, render, smartVidCrop as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISC, LINE, RECT, TEXT = _lib.MARK_DISC, _lib.MARK_LINE, _lib.MARK_RECT, _lib.MARK_TEXT
RED, GREEN = 0, 8


def test_entry_is_declared_bound_and_in_the_history():
    with open(os.path.join(ROOT, 'include', 'svc.h')) as fp:
        header = fp.read()
    assert re.search(r'\bint svc_demo_frames_u8\(const uint8_t \*small', header)
    assert '#define SVC_ABI_VERSION 13' in header and '#define SVC_K_COUNT 14' in header
    history = header[header.index('ABI revision of the loaded library'):header.index('#define SVC_ABI_VERSION')]
    assert re.search(r'\(13, no bump\) svc_demo_frames_u8', history)
    for name, value in (('SVC_MARK_WORDS', _lib.MARK_WORDS), ('SVC_DEMO_MAX_MARKS', _lib.DEMO_MAX_MARKS), ('SVC_MARK_DISC', DISC),
                        ('SVC_MARK_LINE', LINE), ('SVC_MARK_RECT', RECT), ('SVC_MARK_TEXT', TEXT)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert 'svc_demo_frames_u8' in _lib.EXPORTS and 'svc_demo_frames_u8' in _lib.LATER_ENTRIES and _lib.ABI_VERSION == 13
    lib = _lib.load()
    assert lib.svc_abi_version() == 13 and len(lib.svc_demo_frames_u8.argtypes) == 16 and lib.svc_demo_frames_u8.restype is ctypes.c_int


def test_entry_checks_its_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(16)                   # never dereferenced: every call below is a no-op or fails validation first
    ok = dict(small=fake, n=2, ph=9, pw=14, raw=fake, filt=fake, n_maps=1, map_of=fake, marks=fake, n_marks=3, first=fake, atlas=fake,
              atlas_bytes=10, out=fake, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.svc_demo_frames_u8(a['small'], a['n'], a['ph'], a['pw'], a['raw'], a['filt'], a['n_maps'], a['map_of'], a['marks'],
                                      a['n_marks'], a['first'], a['atlas'], a['atlas_bytes'], a['out'], a['flags'], None)
    assert call(n=0) == 0                        # a successful no-op, whatever the pointers
    assert call(n=0, small=None, raw=None, filt=None, map_of=None, marks=None, first=None, atlas=None, out=None) == 0
    for bad in (dict(n=-1), dict(n_maps=-1), dict(n_marks=-1), dict(ph=0), dict(pw=0), dict(ph=-3), dict(flags=2), dict(flags=-1), dict(flags=3),
                dict(small=None), dict(map_of=None), dict(first=None), dict(out=None), dict(raw=None), dict(filt=None), dict(marks=None),
                dict(atlas=None), dict(pw=2 ** 31 // 15 + 1), dict(n=0, ph=0), dict(n=0, flags=4)):
        assert call(**bad) == -1, bad
        assert b'svc_demo_frames_u8' in lib.svc_last_error(), bad


# ---- demo_marks -----------------------------------------------------------------------------------------------------------------
def _vd(fr=25.0):
    """fc = 12 at skip 3: maps of frames 0, 3, 6, 9 and of the last one."""
    bbs = [[100, 0, 302, 350]] * 12
    return dict(fr=fr, fc=12, inds_to_orig=[0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4], h_process=140, w_process=250, h_orig=360, w_orig=640,
                dx=[10.9, 20.0, 30.2, 40.0, 50.0], dy=[5.0, 6.9, 7.0, 8.0, 9.0], dxnf=[10.9, 20.0, 33.9, 40.0, 50.0], dynf=[5.0, 6.9, 7.0, 8.0, 9.0],
                jumps=[255, 7.9, 60, 0, 255], segm_backup=np.array([[0, 6], [7, 11]], np.int32), dxs=[200.7] * 12, dys=[181.0] * 12,
                bbs=bbs, bbs_np=np.asarray(bbs, np.int64))


CP = dict(foces_stab_t=60)


def _frame(marks, first, i, panel=None, kinds=None):
    rows = [tuple(int(v) for v in r) for r in marks[first[i]:first[i + 1]]]
    return [r for r in rows if (panel is None or r[0] >> 8 == panel) and (kinds is None or r[0] & 255 in kinds)]


def _disc(panel, x, y, r, level, shift):
    return (DISC | panel << 8, x, y, 0, 0, r, 0, level << shift)


def _line(x0, y0, x1, y1, t, level, shift):
    return (LINE | 2 << 8, x0, y0, x1, y1, t, 0, level << shift)


def _label(panel, pos, strings):
    _, where = render.demo_atlas()
    rows = []
    for dilated, colour in ((1, 0), (0, 0xffffff)):
        x = pos[0] - 2
        for s in strings:
            off, w, h = where[s]
            rows.append((TEXT | panel << 8, x, pos[1] - (h - 2), 0, 0, off + dilated * w * h, w | h << 16, colour))
            x += w - 4
    return rows


def test_marks_shapes_and_map_index():
    marks, first, map_of = render.demo_marks(_vd(), CP)
    assert marks.dtype == np.int32 and marks.ndim == 2 and marks.shape[1] == 8 and first.dtype == np.int32 and map_of.dtype == np.int32
    assert first.shape == (13,) and first[0] == 0 and first[-1] == len(marks) and (np.diff(first) > 0).all() and (np.diff(first) <= 64).all()
    assert map_of.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4]


def test_trails_lengths_colours_and_the_start_of_the_lists():
    """past_steps = int(25 / 5) = 5: steps j = 1 .. 4 with T = 5 - j, radius 2 + T // 2, level 255 - 20 j - 20; m - j < 0 draws nothing."""
    marks, first, _ = render.demo_marks(_vd(), CP)
    shapes = lambda i: _frame(marks, first, i, panel=2, kinds=(DISC, LINE))
    assert shapes(0) == [_disc(2, 10, 5, 5, 255, GREEN)]                      # frame 0, map 0: nothing behind it
    assert shapes(2) == [_disc(2, 10, 5, 5, 255, GREEN)]                      # frame 2, still map 0: m - 1 < 0 (the reference wraps to the end)
    assert shapes(4) == [_disc(2, 20, 6, 5, 255, GREEN), _disc(2, 10, 5, 4, 215, GREEN)]          # map 1: one step back, no line (m - 2 < 0)
    assert shapes(11) == [_disc(2, 50, 9, 5, 255, GREEN), _disc(2, 40, 8, 4, 215, GREEN), _disc(2, 30, 7, 3, 195, GREEN),
                          _disc(2, 20, 6, 3, 175, GREEN), _disc(2, 10, 5, 2, 155, GREEN),
                          _line(40, 8, 30, 7, 4, 215, GREEN), _line(30, 7, 20, 6, 3, 195, GREEN), _line(20, 6, 10, 5, 2, 175, GREEN)]


def test_red_trail_only_where_the_centres_differ():
    marks, first, _ = render.demo_marks(_vd(), CP)
    red = [_disc(2, 33, 7, 5, 255, RED), _disc(2, 20, 6, 4, 215, RED), _disc(2, 10, 5, 3, 195, RED), _line(20, 6, 10, 5, 4, 215, RED)]
    green = [_disc(2, 30, 7, 5, 255, GREEN), _disc(2, 20, 6, 4, 215, GREEN), _disc(2, 10, 5, 3, 195, GREEN), _line(20, 6, 10, 5, 4, 215, GREEN)]
    for i in (6, 7, 8):                                                      # map 2: dxnf 33.9 != dx 30.2
        assert _frame(marks, first, i, panel=2, kinds=(DISC, LINE)) == red + green, i
    for i in (0, 3, 5, 9, 11):
        assert all(r[7] >> 8 for r in _frame(marks, first, i, panel=2, kinds=(DISC, LINE))), i      # no red anywhere else
    vd = _vd()
    vd['dynf'][3] = 8.5                                                      # y alone differs: red as well
    marks, first, _ = render.demo_marks(vd, CP)
    assert _frame(marks, first, 9, panel=2, kinds=(DISC,))[0] == _disc(2, 40, 8, 5, 255, RED)


def test_jump_score_digits_and_labels():
    marks, first, _ = render.demo_marks(_vd(), CP)
    text = lambda i, panel: _frame(marks, first, i, panel=panel, kinds=(TEXT,))
    cut, jump, title = _label(2, (2, 60), ['orig. cut']), _label(2, (2, 45), ['jump']), _label(2, (2, 15), ['filtered'])
    assert text(0, 2) == _label(2, (2, 30), ['jump:', '2', '5', '5']) + cut + title              # 255: no 'jump'
    assert text(3, 2) == _label(2, (2, 30), ['jump:', '7']) + jump + cut + title                 # '%d' % 7.9
    assert text(6, 2) == _label(2, (2, 30), ['jump:', '6', '0']) + jump + cut + title            # 60 is not below 60: the counter still runs
    assert text(9, 2) == _label(2, (2, 30), ['jump:', '0']) + jump + cut + title
    for panel, s in ((1, 'saliency'), (3, 'overlayed'), (4, 'final')):
        assert text(5, panel) == _label(panel, (2, 15), [s])
    assert text(5, 0) == [] and _frame(marks, first, 5, panel=0) == []
    _, where = render.demo_atlas()
    xs = [r[1] for r in text(0, 2)[:4]]
    assert xs[0] == 0 and np.diff(xs).tolist() == [where['jump:'][1] - 4, where['2'][1] - 4, where['5'][1] - 4]


def test_fade_counters_across_their_last_frame():
    """fade_len = fr = 4, past_steps = 0: 'jump' is set by frames 0 - 2 (map 0, jump 0) and shows on 4 frames from the last of them;
    'orig. cut' is set by every frame index in segm_backup (0, 4, 5, 11)."""
    vd = dict(_vd(fr=4.0), jumps=[0, 255, 255, 255, 255], segm_backup=np.array([[0, 4], [5, 11]], np.int32))
    marks, first, _ = render.demo_marks(vd, CP)
    jump, cut = _label(2, (2, 45), ['jump']), _label(2, (2, 60), ['orig. cut'])
    has = lambda i, label: all(r in _frame(marks, first, i, panel=2, kinds=(TEXT,)) for r in label)
    assert [has(i, jump) for i in range(12)] == [True] * 6 + [False] * 6
    assert [has(i, cut) for i in range(12)] == [True] * 9 + [False, False, True]
    assert _frame(marks, first, 4, panel=2, kinds=(DISC, LINE)) == [_disc(2, 20, 6, 5, 255, GREEN)]      # past_steps 0: no trail at all
    # fr = 25: a counter set once outlives these 12 frames
    marks, first, _ = render.demo_marks(_vd(), CP)
    has = lambda i, label: all(r in _frame(marks, first, i, panel=2, kinds=(TEXT,)) for r in label)
    assert [has(i, jump) for i in range(12)] == [False] * 3 + [True] * 9 and all(has(i, cut) for i in range(12))


def test_overlay_and_final_panels():
    marks, first, _ = render.demo_marks(_vd(), CP)
    for i in (0, 8, 11):
        m = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4][i]
        cx, cy = [(10, 5), (20, 6), (30, 7), (40, 8), (50, 9)][m]
        assert _frame(marks, first, i, panel=3, kinds=(DISC, LINE, RECT)) == [_disc(3, cx, cy, 3, 255, GREEN)]
        # scale_w = 250 / 640, scale_h = 140 / 360: int(200.7 * .390625) = 78, int(181 * .3889) = 70; the window (100, 0, 302, 350) ->
        # int(39.06) + 1, int(0) + 1, int(117.97) - 1, int(136.1) - 1
        assert _frame(marks, first, i, panel=4, kinds=(DISC, LINE, RECT)) == [_disc(4, 78, 70, 3, 255, GREEN),
                                                                               (RECT | 4 << 8, 40, 1, 116, 135, 0, 0, 255 << 8)]


def test_draw_order():
    marks, first, _ = render.demo_marks(_vd(), CP)
    rows = _frame(marks, first, 8)
    order = [(r[0] >> 8, r[0] & 255) for r in rows]
    assert order == [(2, DISC)] * 3 + [(2, LINE)] + [(2, DISC)] * 3 + [(2, LINE)] + [(2, TEXT)] * 10 + [(3, DISC), (4, DISC), (4, RECT)] + \
        [(p, TEXT) for p in (1, 1, 2, 2, 3, 3, 4, 4)]


def test_atlas():
    atlas, where = render.demo_atlas()
    assert atlas.dtype == np.uint8 and atlas.ndim == 1 and render.demo_atlas()[0] is atlas          # once per process
    assert set(where) == set(render.DEMO_STRINGS) >= {'saliency', 'filtered', 'overlayed', 'final', 'jump:', 'jump', 'orig. cut'} | set('0123456789')
    heights = set()
    for s, (off, w, h) in where.items():
        assert 0 <= off and off + 2 * w * h <= len(atlas) and 3 <= w <= 4096 and 3 <= h <= 4096, s
        plain, fat = (atlas[off + k * w * h:off + (k + 1) * w * h].reshape(h, w).astype(int) for k in (0, 1))
        assert plain.max() > 128 and (plain > 0).sum() >= 4, s                          # not empty
        assert not plain[0].any() and not plain[-1].any() and not plain[:, 0].any() and not plain[:, -1].any(), s      # the margin
        pad = np.pad(plain, 1)
        assert np.array_equal(fat, np.max([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)), s
        heights.add(h)
    assert len(heights) == 1                                                            # one line height: strings compose side by side
    spans = sorted((off, off + 2 * w * h) for off, w, h in where.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


# ---- the door -------------------------------------------------------------------------------------------------------------------
def _video():
    return dict(fr=30.0, frame_count=3, w=64, h=36, frames=np.zeros((3, 36, 64, 3), np.uint8), trans_inds=[0, 3])


def test_demo_fn_refusals_come_before_any_work():
    S.set_demo_writer(None)
    with pytest.raises(NotImplementedError, match=r'demo(.|\n)*set_demo_writer\(\)'):
        S.smart_vid_crop(_video(), demo_fn='demo', engine=object())
    with pytest.raises(NotImplementedError, match='demo'):
        S.smart_vid_crop(_video(), demo_fn='demo', engine=object(), stream_batch=8)           # the missing writer is named first
    opened = []
    S.set_demo_writer(lambda *a: opened.append(a))
    try:
        with pytest.raises(ValueError, match='stream_batch'):
            S.smart_vid_crop(_video(), demo_fn='demo', engine=object(), stream_batch=8)
        assert not opened
    finally:
        S.set_demo_writer(None)
    assert S._demo_writer is None


def test_render_demo_needs_the_raw_maps():
    vd = dict(_vd(), smaps_dev=None)
    with pytest.raises(ValueError, match='smaps_orig_dev'):
        render.render_demo(np.zeros((12, 36, 64, 3), np.uint8), vd, CP, engine=object())
    with pytest.raises(ValueError, match='keep_raw'):
        S.after_ingest(dict(xy_stream=None, segmentation=np.zeros((1, 2), np.int32)), CP, object(), keep_raw=True)
