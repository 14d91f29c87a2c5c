"""-m gpu: which bytes every writing entry writes -- all of its output, nothing else.  Every output lies in a poisoned and guarded
buffer (tests/poison.py), every case runs under both fills, every expected value comes from a numpy reference (cv_ref, nv12_ref,
nv12_out_ref, lanczos_ref, tail_ref), never from a device call: a byte that equals its reference under both fills was written, and
the guard bands are checked after every call.  Outputs start at each of the 16 byte phases where the entry takes the caller's
buffer; the shapes are the smallest that reach a row head, a row tail, a last partial group and a second workgroup.  Where no
numpy reference exists (the saliency network, TransNet) the results of the two fills are compared with each other bit for bit:
an unwritten byte would read 0xA5 in one and 0x5A in the other."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nv12_out_ref
import nv12_ref
import poison
from oracle import cv_ref, lanczos_ref, pipeline_ref as P, tail_ref as T, transnet_ref as R
from retargetvid_amd import _lib, ops, synth, transnetv1_handler as Hd, weights
from test_gpu_border import _np_profile
from test_gpu_colour import RENDERS
from test_gpu_parity import _ref_tail

pytestmark = pytest.mark.gpu

N, H, W = 3, 38, 70
DEV = 'cuda'


@pytest.fixture(params=poison.FILLS, ids=['a5', '5a'])
def guard(request, monkeypatch):
    """poison.poisoned_outputs with the fill of the case: the outputs the wrappers allocate themselves are guarded too."""
    p = poison.Poison(request.param)
    monkeypatch.setattr(ops, 'torch', p)
    monkeypatch.setattr(Hd, 'torch', p)
    yield p
    p.check()


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _pictures():
    """Random NV12 frames and the RGB frames they convert to (nv12_ref): one expectation serves both sources."""
    nv = np.random.RandomState(7).randint(0, 256, (N, H * 3 // 2, W)).astype(np.uint8)
    return nv, nv12_ref.nv12_to_rgb(nv, H, W)


def _sources():
    nv, rgb = _pictures()
    return (('rgb24', torch.from_numpy(rgb).to(DEV)), ('nv12', torch.from_numpy(nv).to(DEV)))


def _boxes(bw, bh):
    """Windows at odd origins; the last one touches the frame's corner."""
    b = np.array([[1, 1, 1 + bw, 1 + bh], [3, 5, 3 + bw, 5 + bh], [W - bw, H - bh, W, H]], np.int32)
    assert b.min() >= 0 and (b[:2, :2] & 1).all() and b[:, 2].max() == W and b[:, 3].max() == H
    return b


@functools.lru_cache(maxsize=None)
def _crop(bw, bh, out_hw, interp):
    """The RGB crops [N, oh, ow, 3] of the windows _boxes(bw, bh) by the numpy references."""
    rgb = _pictures()[1]
    wins = [rgb[f, y1:y2, x1:x2] for f, (x1, y1, x2, y2) in enumerate(_boxes(bw, bh).tolist())]
    if out_hw is None or tuple(out_hw) == (bh, bw):
        return np.stack(wins)
    fn = cv_ref.resize_linear_u8 if interp == 'linear' else lanczos_ref.resize_lanczos_u8
    return np.stack([fn(np.ascontiguousarray(x), out_hw[0], out_hw[1]) for x in wins])


def _sinks(crop):
    """(name, keywords, expected bytes) of the sinks the crop's size allows."""
    yield 'rgb', dict(), crop
    yield 'bgr', dict(bgr=True), np.ascontiguousarray(crop[..., ::-1])
    if crop.shape[1] % 2 == 0 and crop.shape[2] % 2 == 0:
        yield 'nv12', dict(out_fmt='nv12'), nv12_out_ref.rgb_to_nv12_fixed(crop)


def _render_into(engine, guard, src, boxes, want, phase, **kw):
    out = guard.empty(want.shape, dtype=torch.uint8, device=DEV, phase=phase)
    assert out.data_ptr() % 16 == phase
    got = engine.render_crops(src, boxes, out=out, **kw)
    assert got is out
    guard.check()
    return np.array_equal(out.cpu().numpy(), want)


# ---- the renderer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('render', RENDERS, ids=lambda r: '%dx%d-%s-%s' % (r[0] + (('%dx%d' % r[1][::-1]) if r[1] else 'copy', r[2])))
def test_renderer_writes_its_output_and_nothing_else_at_every_phase(engine, guard, render):
    """The vector copy, the block copy, INTER_LINEAR and Lanczos up and down; RGB and NV12 sources; RGB, BGR and NV12 sinks; `out` at
    each of the 16 byte phases."""
    (bw, bh), out_hw, interp = render
    crop, boxes = _crop(bw, bh, out_hw, interp), _boxes(bw, bh)
    d_boxes = torch.from_numpy(boxes).to(DEV)
    sinks = list(_sinks(crop))
    assert len(sinks) == 3                                      # every RENDERS size is even
    for fmt, src in _sources():
        for name, kw, want in sinks:
            for phase in range(16):
                ok = _render_into(engine, guard, src, d_boxes, want, phase, out_hw=out_hw, pix_fmt=fmt, interp=interp, **kw)
                assert ok, (fmt, name, phase)


@pytest.mark.parametrize('interp', ops.INTERPS)
def test_renderer_row_widths(engine, guard, interp):
    """ow from 17 to 32: 3 ow mod 16 takes every residue an RGB output row can end on (row_out's bytewise head and tail), at an
    aligned and an odd start; the even ones again with the NV12 sink, whose rows are ow bytes."""
    bw, bh, oh = 31, 17, 24
    d_boxes = torch.from_numpy(_boxes(bw, bh)).to(DEV)
    src = _sources()[0][1]
    seen = set()
    for ow in range(17, 33):
        crop = _crop(bw, bh, (oh, ow), interp)
        seen.add(3 * ow % 16)
        for phase in (0, 9):
            assert _render_into(engine, guard, src, d_boxes, crop, phase, out_hw=(oh, ow), interp=interp), (ow, phase)
            if ow % 2 == 0:
                want = nv12_out_ref.rgb_to_nv12_fixed(crop)
                assert _render_into(engine, guard, src, d_boxes, want, phase, out_hw=(oh, ow), interp=interp, out_fmt='nv12'), (ow, phase, 'nv12')
    assert seen == set(range(16))


# ---- the ingest -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(5, 7), (14, 25)], ids=lambda s: '%dx%d' % s)
def test_ingest_writes_its_output_and_nothing_else_at_every_phase(engine, guard, size):
    sh, sw = size
    want = np.stack([cv_ref.resize_linear_u8(f, sh, sw) for f in _pictures()[1]])
    for (fmt, src), entry in zip(_sources(), ('svc_resize_frames_u8', 'svc_resize_frames_nv12')):
        for phase in range(16):
            out = guard.empty(want.shape, dtype=torch.uint8, device=DEV, phase=phase)
            _lib.check(getattr(engine.lib, entry)(engine._h, _ptr(src), N, H, W, _ptr(out), sh, sw, _stream()))
            guard.check()
            assert np.array_equal(out.cpu().numpy(), want), (fmt, phase)


# ---- the tail -------------------------------------------------------------------------------------------------------------------
def test_threshold_touches_its_range_only(engine, guard):
    """svc_threshold_u8 on [start, start + length) inside 3 x 4096 random bytes: 16 bytes per thread with a bytewise fall-back, so
    every start phase, and lengths around one and two vector words and one workgroup's 4096 bytes."""
    t = 120
    src = np.random.RandomState(1).randint(0, 256, 3 * 4096).astype(np.uint8)
    d_src = torch.from_numpy(src).to(DEV)
    for phase in range(16):
        for length in (0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097):
            buf = guard.empty(src.size, dtype=torch.uint8, device=DEV)
            buf.copy_(d_src)
            a = 4096 + phase
            _lib.check(engine.lib.svc_threshold_u8(engine._h, _ptr(buf, a), length, t, _stream()))
            guard.check()
            want = src.copy()
            seg = want[a:a + length]
            seg[...] = np.where(seg < t, 0, seg)
            assert np.array_equal(buf.cpu().numpy(), want), (phase, length)


def _tail_maps(n, h, w, seed):
    """Raw maps: blobs above both thresholds with soft rims and speckle around them."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    maps = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        m = np.zeros((h, w))
        for _ in range(2 + i % 2):
            cy, cx, ry, rx = rng.uniform(4, h - 4), rng.uniform(4, w - 4), rng.uniform(4, 9), rng.uniform(5, 12)
            m = np.maximum(m, rng.uniform(180, 255) * np.exp(-(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)))
        m = m.astype(np.uint8)
        sp = rng.rand(h, w) < 0.03
        m[sp] = rng.randint(60, 256, int(sp.sum()))
        maps[i] = m
    return maps


def _ref_tail_held(thr, flags, CP):
    """_ref_tail on thresholded maps with SVC_MAP_HELD honoured (include/svc.h): a held map is not filtered, and is blended into
    its successor when it also carries SVC_BLEND_NEXT -> (maps [n, h, w], dx, dy); the centres of held maps mean nothing."""
    hwn = np.ascontiguousarray(np.transpose(thr, (1, 2, 0)))
    for i in range(hwn.shape[2]):
        if not flags[i] & ops.MAP_HELD and CP['clust_filt']:
            hwn[:, :, i] = T.clustering_filt(hwn[:, :, i], CP, {})
        if flags[i] & ops.BLEND_NEXT and i + 1 < hwn.shape[2]:
            hwn[:, :, i + 1] = T.blend_next(hwn[:, :, i], hwn[:, :, i + 1])
    dx, dy = T.centers(hwn, CP)
    return np.transpose(hwn, (2, 0, 1)), dx, dy


TAIL_SETTINGS = {'default': P.init_crop_params(), 'best': P.init_crop_params(True),           # best: factor 4 writes the grown maps back
                 'best_argmax': dict(P.init_crop_params(True), com_km=False), 'no_filter': dict(P.init_crop_params(), clust_filt=False)}


@pytest.mark.parametrize('setting', list(TAIL_SETTINGS))
def test_cluster_center_writes_processed_maps_and_leaves_held_ones(engine, guard, setting):
    """n = 5 maps of 33 x 47 with one HELD | BLEND_NEXT map and one HELD map left for later: processed maps and their centres are
    the oracle's, held maps are byte for byte the input (the centre kernels are launched over all n maps), and nothing lands
    outside maps, xy or stats.  The xy rows of held maps are unspecified (include/svc.h) and not asserted."""
    CP = TAIL_SETTINGS[setting]
    Hm, B = ops.MAP_HELD, ops.BLEND_NEXT
    flags = np.array([B, 0, Hm | B, 0, Hm], np.uint8)
    thr = T.threshold(_tail_maps(5, 33, 47, seed=21).copy(), CP['t_threshold'])
    assert all(np.count_nonzero(m) > CP['hdbscan_min'] + 2 for m in thr)
    ref_maps, dx, dy = _ref_tail_held(thr, flags, CP)
    plain = _ref_tail(thr, (flags & B).astype(bool), CP)                 # the statement above is _ref_tail's where nothing is held
    none_held = _ref_tail_held(thr, flags & B, CP)
    assert np.array_equal(none_held[0], plain[0]) and none_held[1:] == plain[1:3]
    if CP['clust_filt']:
        assert not np.array_equal(ref_maps[[0, 1, 3]], thr[[0, 1, 3]])   # the filter changes the processed maps
    assert np.array_equal(ref_maps[[2, 4]], thr[[2, 4]])
    maps = guard.empty(thr.shape, dtype=torch.uint8, device=DEV)
    maps.copy_(torch.from_numpy(thr).to(DEV))
    xy, stats = engine.cluster_center_(maps, flags, CP, want_stats=True)
    guard.check()
    got, xy, stats = maps.cpu().numpy(), xy.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(got[[2, 4]], thr[[2, 4]])
    assert np.array_equal(got, ref_maps)
    for i in (0, 1, 3):
        if dx[i] is None:
            assert np.isnan(xy[i]).all(), i
        else:
            assert xy[i, 0] == dx[i] and xy[i, 1] == dy[i], i
    assert stats.shape == (5, 4) and (stats[[0, 1, 3], 0] > 0).all()       # points of the processed maps


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_iou_writes_n_values(engine, guard, n):
    rng = np.random.RandomState(n)
    a = rng.randint(-5, 600, (n, 4)).astype(np.int32); a[:, 2:] += np.abs(a[:, :2])
    b = rng.randint(-5, 600, (n, 4)).astype(np.int32); b[:, 2:] += np.abs(b[:, :2])
    got = ops.iou_boxes(a, b)
    guard.check()
    assert np.array_equal(got, np.array([T.iou(x, y) for x, y in zip(a.tolist(), b.tolist())]))


# ---- the network's outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(35, 35), (20, 300), (3, 1100)], ids=lambda s: '%dx%d' % s)
def test_border_profile_beyond_one_column_per_thread(engine, guard, shape):
    """svc_border_profile_u8 at widths above 256 (a second column per thread) and above 1024 (the loop over column groups)."""
    h, w = shape
    rng = np.random.RandomState(h + w)
    maps = np.where(rng.rand(3, h, w) < 0.05, rng.randint(1, 256, (3, h, w)), 0).astype(np.uint8)
    maps[1, :, w - 1] = 0
    maps[2, h - 1, :] = 0
    maps[0, 0, w - 1] = 255
    want = _np_profile(maps)
    assert want.min() == 0 and want[:, h:].max() == 255
    got = engine.border_profile(torch.from_numpy(maps).to(DEV))
    guard.check()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


def test_saliency_entries_write_every_byte_of_their_maps(engine):
    """svc_saliency_u8, _thresholded_u8, _census_u8 and _profile_u8 on n = 3 frames of 141 x 249 (n h w is no multiple of 16),
    `out` at phases 0 and 1, under both fills: the raw maps are the same bytes every time, the thresholded ones numpy's threshold
    of them, census and profile rows numpy's on the raw maps, and no guard is touched."""
    n, h, w, t = 3, 141, 249, 120
    assert n * h * w % 16
    fr = torch.from_numpy(synth.blob_frames(n, h, w, seed=5)).to(DEV)
    raws = []
    for fill in poison.FILLS:
        g = poison.Poison(fill)
        for phase in (0, 1):
            def out():
                return g.empty((n, h, w), dtype=torch.uint8, device=DEV, phase=phase)
            raw = engine.saliency(fr, out=out()).cpu().numpy()
            g.check()
            raws.append(raw)
            thr = np.where(raw < t, 0, raw)
            assert thr.any() and not np.array_equal(thr, raw)
            census = np.stack([(raw == v).sum((1, 2)) for v in (t - 1, t, t + 1)], 1)
            assert census.any()
            m = engine.saliency(fr, out=out(), threshold=t)
            g.check()
            assert np.array_equal(m.cpu().numpy(), thr), (fill, phase, 'thresholded')
            c = g.zeros((n, 4), dtype=torch.int32, device=DEV)
            m = engine.saliency(fr, out=out(), threshold=t, census=c)
            g.check()
            assert np.array_equal(m.cpu().numpy(), thr), (fill, phase, 'census')
            assert np.array_equal(c.cpu().numpy()[:, :3], census), (fill, phase, 'census')
            c, p = g.zeros((n, 4), dtype=torch.int32, device=DEV), g.zeros((n, h + w), dtype=torch.int32, device=DEV)
            m = engine.saliency(fr, out=out(), threshold=t, census=c, profile=p)
            g.check()
            assert np.array_equal(m.cpu().numpy(), thr), (fill, phase, 'profile')
            assert np.array_equal(c.cpu().numpy()[:, :3], census), (fill, phase, 'profile')
            assert np.array_equal(p.cpu().numpy(), _np_profile(raw)), (fill, phase, 'profile')
    assert all(np.array_equal(r, raws[0]) for r in raws[1:])            # the same under both fills: every byte was written
    assert len(np.unique(raws[0])) > 16


def test_transnet_writes_its_rows(engine):
    """svc_transnet_predict and _predict_rows on 3 windows of T = 17, rows (3, 12), on the default pipe, under both fills: the full
    pass is the oracle's within the tolerance of test_gpu_transnet and the same bits under both fills, the kept rows are bit for
    bit the full pass, and the guards round probs hold.  The rows outside the kept range are unspecified and not asserted."""
    sd = weights.make_transnet_state_dict(0)
    rng = np.random.RandomState(17)
    fr = rng.randint(0, 256, (3, 17, 27, 48, 3)).astype(np.uint8)
    d = torch.from_numpy(fr).to(DEV)
    ref = R.forward(sd, fr)
    net = Hd.ShotTransNet(Hd.ShotTransNetParams(), weights=sd, engine=engine)
    fulls = []
    try:
        for fill in poison.FILLS:
            g = poison.Poison(fill)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(Hd, 'torch', g)
                full = net.predict_raw_device(d)
                g.check()
                part = net.predict_raw_device(d, rows=(3, 12))
                g.check()
            assert g.allocations == 2
            full, part = full.cpu().numpy(), part.cpu().numpy()
            assert full.shape == (3, 17) and np.abs(full - ref).max() <= 1e-4, (fill, float(np.abs(full - ref).max()))
            assert np.array_equal(part[:, 3:12], full[:, 3:12]), fill
            fulls.append(full)
    finally:
        net.close()
    assert np.array_equal(fulls[0], fulls[1])
