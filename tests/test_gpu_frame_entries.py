"""-m gpu: which C entry each argument combination of Engine.resize_frames / render_crops / render_windows reaches.  The entries give
the same bytes on the same pictures, so no byte test can tell them apart -- but they run different kernel instances (the packed
entries are the measured default path), and the order in which ops.Engine picks one is part of its contract:
    render:  out_layout -> svc_render_crops_to_layout | a colour -> svc_render_crops_colour | interp != 'linear' -> svc_render_crops_filter
             | layout -> svc_render_crops_layout | else ops.RENDER_ENTRIES[pix_fmt, out_fmt]
    resize:  a colour -> svc_resize_frames_colour | layout -> svc_resize_frames_layout | else svc_resize_frames_nv12 / _u8
A colour that spells out BT.601 limited is no colour.  eng.lib is wrapped in a proxy that notes the name of every svc_resize_frames_* /
svc_render_* function called and forwards the call; every case must make exactly one such call, and (a layout here holds the packed
values, so) return the bytes of the plain call on the same pictures."""
import numpy as np
import pytest
import torch

from retargetvid_amd import ops

pytestmark = pytest.mark.gpu

N, H, W = 2, 36, 64
BW = BH = 16
OUT_HWS = ((20, 30), None)                      # resampled (even: legal for NV12) | the copy at the window size
BOXES = np.array([[2, 4, 2 + BW, 4 + BH], [W - BW, H - BH, W, H]], np.int32)
ORIGINS = BOXES[:, :2] * 256                    # the same windows for render_windows: whole pixels
BT601, BT709 = ('bt601', 'limited'), ('bt709', 'full')
FMTS = [(p, o) for p in ops.PIX_FMTS for o in ops.OUT_FMTS]


class Recorder:
    """eng.lib, noting the frame I/O entries that are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(('svc_resize_frames_', 'svc_render_')):
            return fn

        def noted(*args):
            self.calls.append(name)
            return fn(*args)
        return noted


@pytest.fixture
def rec(engine, monkeypatch):
    r = Recorder(engine.lib)
    monkeypatch.setattr(engine, 'lib', r)
    return r


_SRC = {}


def _frames(fmt):
    if fmt not in _SRC:
        _SRC[fmt] = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (N,) + ops.frame_shape(fmt, H, W)).astype(np.uint8)).cuda()
    return _SRC[fmt]


def _reached(rec, call, *args, **kw):
    """The one entry `call(*args, **kw)` reaches, and its result."""
    del rec.calls[:]
    out = call(*args, **kw)
    assert len(rec.calls) == 1, (kw, rec.calls)
    return rec.calls[0], out


def _in(fmt, layout):
    """frames and layout= of a case: packed, or the same bytes as [n, frame_stride] under the layout of the packed values."""
    f = _frames(fmt)
    return (f.reshape(N, -1), ops.frame_layout(fmt, H, W)) if layout else (f, None)


@pytest.mark.parametrize('fmt', ops.PIX_FMTS)
def test_resize_ladder(engine, rec, fmt):
    def run(layout=False, colour=None):
        f, lay = _in(fmt, layout)
        return _reached(rec, engine.resize_frames, frames=f, sh=14, sw=25, pix_fmt=fmt, layout=lay, colour=colour)

    plain = 'svc_resize_frames_nv12' if fmt == 'nv12' else 'svc_resize_frames_u8'
    name, want = run()
    assert name == plain
    cases = [(dict(layout=True), 'svc_resize_frames_layout', True)]
    if fmt == 'nv12':
        cases += [(dict(colour=BT709), 'svc_resize_frames_colour', False),
                  (dict(colour=BT709, layout=True), 'svc_resize_frames_colour', False),
                  (dict(colour=BT601), plain, True),                                          # spelled out: the call without it
                  (dict(colour=dict(matrix='smpte170m', range='tv')), plain, True),
                  (dict(colour=BT601, layout=True), 'svc_resize_frames_layout', True)]
    for kw, entry, same in cases:
        name, got = run(**kw)
        assert name == entry, (kw, name)
        assert torch.equal(got, want) == same, kw


@pytest.mark.parametrize('out_hw', OUT_HWS, ids=['resample', 'copy'])
@pytest.mark.parametrize('pix_fmt,out_fmt', FMTS)
def test_render_ladder(engine, rec, pix_fmt, out_fmt, out_hw):
    oh, ow = out_hw or (BH, BW)

    def run(layout=False, out_layout=False, **kw):
        f, lay = _in(pix_fmt, layout)
        olay = ops.frame_layout(out_fmt, oh, ow) if out_layout else None
        name, out = _reached(rec, engine.render_crops, frames=f, boxes=BOXES, out_hw=out_hw, pix_fmt=pix_fmt, out_fmt=out_fmt, layout=lay,
                             out_layout=olay, **kw)
        return name, out.reshape((N,) + ops.frame_shape(out_fmt, oh, ow))

    # the colours a side may be given: only an NV12 side takes one
    cin, cout = pix_fmt == 'nv12', out_fmt == 'nv12'
    other = [dict(colour=BT709)] * cin + [dict(out_colour=BT709)] * cout + [dict(colour=BT709, out_colour=BT709)] * (cin and cout)
    spelled = [dict(colour=BT601)] * cin + [dict(out_colour=dict(matrix='bt470bg', range='mpeg'))] * cout

    want = {}
    for interp in ops.INTERPS:
        below = 'svc_render_crops_filter' if interp == 'lanczos' else None     # the rung a call with this filter lands on at the latest
        name, want[interp] = run(interp=interp)
        assert name == (below or ops.RENDER_ENTRIES[pix_fmt, out_fmt])
        cases = [(dict(layout=True), below or 'svc_render_crops_layout', True),
                 (dict(out_layout=True), 'svc_render_crops_to_layout', True),
                 (dict(out_layout=True, layout=True), 'svc_render_crops_to_layout', True)]
        for c in other:
            cases += [(c, 'svc_render_crops_colour', False), (dict(c, layout=True), 'svc_render_crops_colour', False),
                      (dict(c, layout=True, out_layout=True), 'svc_render_crops_to_layout', False)]
        for c in spelled:
            cases += [(c, below or ops.RENDER_ENTRIES[pix_fmt, out_fmt], True), (dict(c, layout=True), below or 'svc_render_crops_layout', True),
                      (dict(c, out_layout=True), 'svc_render_crops_to_layout', True)]
        if out_fmt == 'rgb24':
            cases += [(dict(bgr=True), below or ops.RENDER_ENTRIES[pix_fmt, out_fmt], False)]
        for kw, entry, same in cases:
            name, got = run(interp=interp, **kw)
            assert name == entry, (interp, kw, name)
            assert torch.equal(got, want[interp]) == same, (interp, kw)
    if out_hw is None:
        assert torch.equal(want['lanczos'], want['linear'])                  # the window size is the exact copy either way

    # sub-pixel windows: one entry for everything; at whole-pixel origins the bytes of render_crops
    origins = torch.from_numpy(ORIGINS).cuda()
    for kw in [dict(), dict(layout=True), dict(out_layout=True), dict(layout=True, out_layout=True)] + spelled + other:
        kw = dict(kw)
        f, lay = _in(pix_fmt, kw.pop('layout', False))
        olay = ops.frame_layout(out_fmt, oh, ow) if kw.pop('out_layout', False) else None
        name, got = _reached(rec, engine.render_windows, frames=f, origins_q8=origins, win_wh=(BW, BH), out_hw=out_hw, pix_fmt=pix_fmt,
                             out_fmt=out_fmt, layout=lay, out_layout=olay, **kw)
        assert name == 'svc_render_windows_q8', kw
        if kw not in other:
            assert torch.equal(got.reshape(want['linear'].shape), want['linear']), kw


def test_render_direct(engine, rec):
    """Engine._render, the door the pipeline and the benchmarks use with their own output buffer: the same ladder."""
    boxes = torch.from_numpy(BOXES).cuda()
    for pix_fmt, out_fmt in FMTS:
        out = torch.empty((N,) + ops.frame_shape(out_fmt, 20, 30), dtype=torch.uint8, device='cuda')
        args = (_frames(pix_fmt), boxes, BW, BH, out, False, pix_fmt, out_fmt)
        assert _reached(rec, engine._render, *args)[0] == ops.RENDER_ENTRIES[pix_fmt, out_fmt]
        assert _reached(rec, engine._render, *args, None, 'lanczos')[0] == 'svc_render_crops_filter'
