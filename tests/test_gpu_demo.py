"""-m gpu: the five-panel demo frames -- svc_demo_frames_u8 / ops.demo_frames against the NumPy restatement of include/svc.h's
rules (tests/demo_cases.py), exact on every byte, into poisoned and guarded outputs at every phase; then render.render_demo and
the demo_fn door of smart_vid_crop end to end."""
import numpy as np
import pytest
import torch

import demo_cases as D
from poison import FILL, Poison, poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from retargetvid_amd import ops, render, smartVidCrop as S, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

SHAPES = ((9, 14), (8, 16), (35, 62), (140, 250))       # (9, 14): a row of 210 bytes, no row start 16-aligned


def _shifted(a, phase, fill=0xEE):
    """The array on the device at an address `phase` bytes past a 16-aligned one (inputs need no alignment)."""
    a = np.ascontiguousarray(a)
    raw = np.concatenate([np.full(phase, fill, np.uint8), a.view(np.uint8).reshape(-1)])
    t = torch.from_numpy(raw).cuda()[phase:]
    return t.view(torch.from_numpy(a).dtype).view(a.shape) if a.size else torch.from_numpy(a).cuda()


def _run(small, raw, filt, map_of, marks, first, atlas, bgr=False, phase=0, in_phase=0):
    """One call into a poisoned, guarded output at `phase` -> the bytes; the inputs must come back unchanged and the guards whole."""
    P = Poison()
    n, ph, pw, _ = small.shape
    host = [small, raw, filt, np.asarray(map_of, np.int32), np.asarray(marks, np.int32).reshape(-1, 8), np.asarray(first, np.int32)]
    dev = [_shifted(h, in_phase if h.dtype == np.uint8 else 0) for h in host]
    at = None if atlas is None else _shifted(atlas, in_phase)
    out = P.empty((n, ph, 5 * pw, 3), dtype=torch.uint8, device='cuda', phase=phase)
    got = ops.demo_frames(*dev, at, bgr=bgr, out=out)
    assert got is out
    res = out.cpu().numpy()
    P.check()
    for h, d in zip(host, dev):
        assert np.array_equal(d.cpu().numpy(), h), 'an input changed'
    if atlas is not None:
        assert np.array_equal(at.cpu().numpy(), atlas)
    return res


def _assert_same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        f, y, x, c = bad[0]
        raise AssertionError('%s: %d bytes differ, first at frame %d row %d column %d (panel %d) channel %d: got %d, expected %d'
                             % (what, len(bad), f, y, x, x // (got.shape[2] // 5), c, got[f, y, x, c], exp[f, y, x, c]))


@pytest.mark.parametrize('ph,pw', SHAPES)
@pytest.mark.parametrize('n', (1, 5, 33))
def test_random_marks_every_shape(ph, pw, n):
    n_maps = max(1, n // 2)
    small, raw, filt, atlas = D.inputs(n, ph, pw, n_maps, seed=ph + n)
    marks, first = D.random_marks(n, ph, pw, len(atlas), seed=pw + n)
    map_of = np.arange(n) % n_maps
    map_of[::5] = (-1, n_maps)[n % 2]
    if n > 2:
        map_of[2] = n_maps if n % 2 == 0 else -1
    exp = D.compose(small, raw, filt, map_of, marks, first, atlas)
    combos = ((0, False), (1, True), (8, False)) if n != 5 else ((0, True), (1, False), (8, True), (15, False))
    for phase, bgr in combos:
        got = _run(small, raw, filt, map_of, marks, first, atlas, bgr=bgr, phase=phase, in_phase=(phase * 7 + 3) % 16)
        _assert_same(got, exp[..., ::-1] if bgr else exp, (ph, pw, n, phase, bgr))


@pytest.mark.parametrize('ph,pw', SHAPES[:3])
def test_every_kind_inside_and_across_every_panel_edge(ph, pw):
    """One frame per (kind, panel): nine marks, inside and across each edge and corner.  A mark never shows in a neighbour: outside
    its panel's columns the frame is the one without marks."""
    small, raw, filt, atlas = D.inputs(20, ph, pw, 3, seed=11)
    map_of = np.arange(20) % 3
    lists = [D.edge_marks(kind, panel, ph, pw) for kind in (D.DISC, D.LINE, D.RECT, D.TEXT) for panel in range(5)]
    marks, first = D.frames_of(lists)
    exp = D.compose(small, raw, filt, map_of, marks, first, atlas)
    bare = D.compose(small, raw, filt, map_of, marks[:0], np.zeros(21, np.int32), atlas)
    got = _run(small, raw, filt, map_of, marks, first, atlas, phase=1)
    _assert_same(got, exp, (ph, pw))
    for f in range(20):
        panel = f % 5
        cols = np.ones(5 * pw, bool)
        cols[panel * pw:(panel + 1) * pw] = False
        assert np.array_equal(got[f][:, cols], bare[f][:, cols]), (f, 'a mark shows outside its panel')
        assert not np.array_equal(got[f][:, ~cols], bare[f][:, ~cols]), (f, 'the marks of this frame drew nothing')


@pytest.mark.parametrize('ph,pw', ((9, 14), (35, 62)))
def test_special_marks(ph, pw):
    small, raw, filt, atlas = D.inputs(16, ph, pw, 2, seed=5)
    F = D.special_frames(ph, pw, len(atlas))
    names = sorted(F)
    marks, first = D.frames_of([F[k] for k in names])
    n = len(names)
    small, map_of = small[:n], np.arange(n) % 2
    exp = D.compose(small, raw, filt, map_of, marks, first, atlas)
    bare = D.compose(small, raw, filt, map_of, marks[:0], np.zeros(n + 1, np.int32), atlas)
    for phase, bgr in ((0, False), (8, True)):
        got = _run(small, raw, filt, map_of, marks, first, atlas, bgr=bgr, phase=phase)
        _assert_same(got, exp[..., ::-1] if bgr else exp, (ph, pw, phase, bgr))
    # the restatement itself says what these cases are about
    i = names.index('ignored')
    changed = np.argwhere((exp[i] != bare[i]).any(axis=2))
    assert 0 < len(changed) <= 5 and (changed[:, 0] <= 2).all() and (changed[:, 1] >= 4 * pw).all()      # only the last disc (radius 1, panel 4) applies
    i = names.index('seventy')
    only64 = D.compose(small[i:i + 1], raw, filt, map_of[i:i + 1], np.asarray(F['seventy'][:64]), [0, 64], atlas)
    assert np.array_equal(exp[i], only64[0]) and len(F['seventy']) == 70
    i = names.index('overlap')
    flipped = D.compose(small[i:i + 1], raw, filt, map_of[i:i + 1], np.asarray(F['overlap'][::-1]), [0, len(F['overlap'])], atlas)
    assert not np.array_equal(exp[i], flipped[0])               # the order matters, and the kernel has the list's


def test_first_not_monotone_and_out_of_range():
    ph, pw, n = 9, 14, 6
    small, raw, filt, atlas = D.inputs(n, ph, pw, 2, seed=8)
    marks, _ = D.random_marks(12, ph, pw, len(atlas), seed=3, per_frame=6)
    k = len(marks)
    for first in ([5, 2, 9, 9, 0, k, 3], [0, k + 7, -4, k, k // 2, 10 ** 6, -10 ** 6], [k, 0, k, 0, k, 0, k]):
        exp = D.compose(small, raw, filt, [0, 1, -1, 2, 0, 1], marks, first, atlas)
        got = _run(small, raw, filt, [0, 1, -1, 2, 0, 1], marks, first, atlas, phase=1)
        _assert_same(got, exp, first)


def test_null_atlas_null_marks_and_no_maps():
    ph, pw, n = 8, 16, 3
    small, raw, filt, atlas = D.inputs(n, ph, pw, 2, seed=9)
    marks, first = D.frames_of([[D.mark(D.DISC, 2, 4, 4, 0, 0, 2, 0, (1, 2, 3))], [D.mark(D.RECT, 0, 1, 1, 9, 6)], [D.mark(D.LINE, 4, 0, 0, 15, 7, 2)]])
    _assert_same(_run(small, raw, filt, [0, 1, 0], marks, first, None), D.compose(small, raw, filt, [0, 1, 0], marks, first, None), 'no atlas')
    text = np.asarray([D.mark(D.TEXT, 1, 0, 0, 0, 0, 0, 4 | 4 << 16)], np.int32)                  # a TEXT mark without an atlas: left alone
    _assert_same(_run(small, raw, filt, [0, 1, 0], text, [0, 1, 1, 1], None), D.compose(small, raw, filt, [0, 1, 0], text, [0, 1, 1, 1], None), 'text, no atlas')
    none = np.zeros((0, 8), np.int32)
    _assert_same(_run(small, raw, filt, [1, 1, 5], none, [0, 0, 0, 0], atlas), D.compose(small, raw, filt, [1, 1, 5], none, [0, 0, 0, 0], atlas), 'no marks')
    _assert_same(_run(small, raw[:0], filt[:0], [0, 0, 0], marks, first, atlas), D.compose(small, raw[:0], filt[:0], [0, 0, 0], marks, first, atlas), 'no maps')
    assert tuple(ops.demo_frames(torch.from_numpy(small[:0]).cuda(), torch.from_numpy(raw).cuda(), torch.from_numpy(filt).cuda(),
                                 np.zeros(0, np.int32), none, np.zeros(1, np.int32), None).shape) == (0, ph, 5 * pw, 3)


def test_overlay_on_every_value_pair():
    """Panel 3 on all 256 x 256 pairs (picture value = the row, map value = the column) in one call: np.rint of the mean, i.e. ties to even."""
    v = np.arange(256, dtype=np.uint8)
    small = np.ascontiguousarray(np.broadcast_to(v[None, :, None, None], (1, 256, 256, 3)))
    filt = np.ascontiguousarray(np.broadcast_to(v[None, None, :], (1, 256, 256)))
    raw = np.zeros_like(filt)
    got = _run(small, raw, filt, [0], np.zeros((0, 8), np.int32), [0, 0], None)
    a, b = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing='ij')
    exp = np.rint((a + b) / 2).astype(np.uint8)
    for c in range(3):
        assert np.array_equal(got[0, :, 3 * 256:4 * 256, c], exp)
    assert np.array_equal(got[0, :, :256], small[0]) and np.array_equal(got[0, :, 4 * 256:], small[0])
    assert not got[0, :, 256:512].any() and np.array_equal(got[0, :, 512:768, 1], filt[0])


def test_ops_checks_before_any_device_work():
    small = torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device='cuda')
    maps = torch.zeros((1, 8, 16), dtype=torch.uint8, device='cuda')
    ok = dict(small=small, raw=maps, filt=maps, map_of=[0, 0], marks=np.zeros((0, 8), np.int32), first=[0, 0, 0], atlas=None)
    for bad in (dict(small=small.cpu()), dict(small=small[:, :, :, :2]), dict(raw=maps[:, :4]), dict(filt=maps.to(torch.int32)), dict(map_of=[0]),
                dict(marks=np.zeros((3, 7), np.int32)), dict(first=[0, 0]), dict(atlas=np.zeros((2, 2), np.uint8)),
                dict(out=torch.zeros((2, 8, 80, 4), dtype=torch.uint8, device='cuda')), dict(first=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.demo_frames(**dict(ok, **bad))


# ---- end to end --------------------------------------------------------------------------------------------------------

class _Recorder:
    def __init__(self, log, *args):
        self.log = log
        log.update(args=args, frames=[], released=0)

    def write(self, f):
        self.log['frames'].append(np.array(f))

    def release(self):
        self.log['released'] += 1


@pytest.fixture(scope='module')
def demo_run(engine):
    """smart_vid_crop on a 64 x 36 video of 40 frames with two cuts, best settings, with and without demo_fn."""
    torch.set_num_threads(8)
    video = dict(fr=25.0, frame_count=40, w=64, h=36, frames=synth.blob_frames(40, 36, 64, seed=6), trans_inds=[0, 13, 27, 40])
    CP = S.sc_init_crop_params(use_best_settings=True)
    log = {}
    S.set_demo_writer(lambda path, fr, size: _Recorder(log, path, fr, size))
    try:
        VD, res = S.smart_vid_crop(video, dict(CP), demo_fn='demo_clip', engine=engine)
    finally:
        S.set_demo_writer(None)
    VD0, res0 = S.smart_vid_crop(video, dict(CP), engine=engine)
    return video, CP, VD, res, VD0, res0, log


def _restated(video_frames_small, VD, CP):
    marks, first, map_of = render.demo_marks(VD, CP)
    atlas, _ = render.demo_atlas()
    return D.compose(video_frames_small, VD['smaps_orig_dev'].cpu().numpy(), VD['smaps_dev'].cpu().numpy(), map_of, marks, first, atlas)


def test_demo_door_end_to_end(engine, demo_run):
    video, CP, VD, res, VD0, res0, log = demo_run
    ph, pw = int(VD['h_process']), int(VD['w_process'])
    assert log['args'] == ('demo_clip', 25.0, (5 * pw, ph)) and log['released'] == 1 and len(log['frames']) == 40 and 't_demo' in res
    written = np.stack(log['frames'])
    got = render.render_demo(video, VD, CP, engine=engine)
    assert got.shape == (40, ph, 5 * pw, 3) and np.array_equal(written, got)
    small = engine.resize_frames(torch.from_numpy(video['frames']).cuda(), ph, pw).cpu().numpy()
    _assert_same(got, _restated(small, VD, CP), 'render_demo against the restatement fed from VD')
    assert np.array_equal(got[:, :, :pw], small)
    # panels 1 and 2 away from their marks: the maps themselves (the titles, the trail and the scores cover part of them)
    m = np.asarray(VD['inds_to_orig'][:40])
    raw, filt = VD['smaps_orig_dev'].cpu().numpy()[m], VD['smaps_dev'].cpu().numpy()[m]
    marks, first, map_of = render.demo_marks(VD, CP)
    assert np.array_equal(map_of, m)
    bare = D.compose(small, VD['smaps_orig_dev'].cpu().numpy(), VD['smaps_dev'].cpu().numpy(), map_of, marks[:0], np.zeros(41, np.int32), None)
    assert np.array_equal(bare[:, :, pw:2 * pw, 0], raw) and np.array_equal(bare[:, :, 2 * pw:3 * pw, 2], filt)
    untouched = (got == bare).all(axis=3)
    assert untouched[:, :, pw:3 * pw].mean() > 0.5 and not untouched.all()
    for c in range(3):
        assert np.array_equal(got[:, :, pw:2 * pw, c][untouched[:, :, pw:2 * pw]], raw[untouched[:, :, pw:2 * pw]])
        assert np.array_equal(got[:, :, 2 * pw:3 * pw, c][untouched[:, :, 2 * pw:3 * pw]], filt[untouched[:, :, 2 * pw:3 * pw]])
    # the analysis is the one without a demo
    assert VD['bbs'] == VD0['bbs'] and 'smaps_orig_dev' not in VD0
    timing = lambda r: {k: v for k, v in r.items() if not k.startswith('t_')}
    assert timing(res) == timing(res0)
    # chunks and a sink; BGR
    seen = []
    assert render.render_demo(video, VD, CP, engine=engine, chunk=16, sink=lambda c: seen.append(c.copy())) is None
    assert [len(c) for c in seen] == [16, 16, 8] and np.array_equal(np.concatenate(seen), got)
    assert np.array_equal(render.render_demo(video, VD, CP, engine=engine, bgr=True, chunk=7), got[..., ::-1])
    with pytest.raises(ValueError):
        render.render_demo(video, VD0, CP, engine=engine)


def test_demo_from_an_nv12_pitched_source(engine, demo_run):
    from nv12_ref import nv12_to_rgb, rgb_to_nv12
    video, CP, VD = demo_run[:3]
    h, w, pitch, coded_h = 36, 64, 128, 48
    nv = rgb_to_nv12(video['frames'])
    buf = np.full((40, coded_h * 3 // 2, pitch), 0xFF, np.uint8)
    buf[:, :h, :w] = nv[:, :h]
    buf[:, coded_h:coded_h + h // 2, :w] = nv[:, h:]
    L = ops.frame_layout('nv12', h, w, dict(pitch=pitch, chroma_offset=pitch * coded_h), pitch * coded_h * 3 // 2)
    surfaces = dict(video, frames=buf.reshape(40, -1), pix_fmt='nv12', layout=L)
    converted = dict(video, frames=nv12_to_rgb(nv, h, w))
    a = render.render_demo(surfaces, VD, CP, engine=engine, chunk=16)
    b = render.render_demo(converted, VD, CP, engine=engine, chunk=16)
    assert np.array_equal(a, b) and not np.array_equal(b[:, :, :int(VD['w_process'])], b[:, :, :int(VD['w_process'])] * 0)
