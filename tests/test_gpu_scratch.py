"""-m gpu: no pass of the library rides what an earlier call left in the handle's scratch.

A handle keeps its workspaces from call to call at the same addresses (DevBuf::ensure only grows), so a kernel that reads a value its
own pass should have written reads the previous call's -- and a test that compares two calls on one handle has often made that the
right value.  The library's test switch (svc_debug_scratch_fill; csrc/svc_internal.h lists what is scratch) fills the scratch before
every pass; poison.poisoned_workspaces turns it on with 0xFF for every test of the modules that opt in.  Here, directed:

  * the saliency network and TransNet under three settings -- off, 0xFF (NaN in fp32 and in every bf16 plane) and 0x7F (3.39e38: a
    ReLU6 clamp turns a stale NaN into an exact 0 and a max-pool ignores it; 3.39e38 clamps to 6 and wins a maximum) -- after a decoy
    call that left other values behind: bit for bit the results of a handle that has seen nothing else;
  * TransNet's kept-rows pass (what production runs) after a decoy FULL pass over other windows of the same length and count, so that
    everything outside the frames it computes holds plausible values of another input; every tap inside the float64 GATES of
    tests/test_gpu_transnet_layers.py;
  * the tail by history, not by byte (its workspace holds indices and counts and is filled with zeros whatever the byte): case X on
    a fresh handle and on a handle whose previous call was a decoy D that is larger than X in one directed way;
  * the switch itself.

Every comparison is bit equality between two runs of the device (floats through their uint32 image), or reuses GATES."""
import functools
import os

import numpy as np
import pytest
import torch

from poison import WS_FILL, WS_SETTINGS, poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import cv_ref, pipeline_ref as P, tail_ref as T, transnet_ref as R
from retargetvid_amd import ops, weights
from retargetvid_amd._lib import SvcError
from test_gpu_parity import _ref_tail, _state_is_the_oracles
from test_gpu_transnet_layers import KEPT, LAYERS, PIPES, check_layers, computed_frames, make_net, oracle as shot_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]


def bits(a):
    """The bytes of an array as integers: equality that a NaN does not escape."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8, 2: np.uint16}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the saliency network ---------------------------------------------------------------------------------------------------
NET_SHAPES = [(140, 250), (250, 140), (8, 8), (19, 250)]
NET_COUNTS = {(8, 8): (1, 3, 33)}                  # 33 frames: two chunks of the default 32
ENTRIES = ('plain', 'threshold', 'census', 'profile')
DECOY_SHAPE = (187, 250)                           # a 288 x 384 network input: more floats per frame than any case's
NET_TAPS = (('FEAT4X', 8, 64), ('FEAT2X', 16, 160), ('FEAT1X', 32, 1296), ('POSTCNN', 32, 256), ('DEC', 8, 64), ('PRE', None, None))


@functools.lru_cache(maxsize=None)
def _layers():
    return weights.fold_state_dict(weights.make_synthetic_state_dict(0))


def _net_engine(pipe, front):
    env = {'SVC_MX': pipe, 'SVC_FRONT': front}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = ops.Engine.from_layers(_layers())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert eng.matrix_pipe() == pipe
    return eng


@pytest.fixture(scope='module')
def net_engines():
    """One long-lived handle per (matrix pipe, SVC_FRONT): the handle under test, dirtier with every case."""
    made = {}

    def get(pipe, front):
        if (pipe, front) not in made:
            made[pipe, front] = _net_engine(pipe, front)
        return made[pipe, front]
    yield get
    for e in made.values():
        e.close()


def _run_entry(eng, fr, entry):
    """One saliency call through `entry` -> {name: array}: the u8 maps, the census / profile rows where the entry has them, and the
    six taps of every frame of the call's last pass."""
    n, h, w, _ = fr.shape
    kw = {}
    if entry != 'plain':
        kw['threshold'] = 120
    if entry in ('census', 'profile'):
        kw['census'] = torch.zeros((n, 4), dtype=torch.int32, device='cuda')
    if entry == 'profile':
        kw['profile'] = torch.zeros((n, h + w), dtype=torch.int32, device='cuda')
    out = {'maps': eng.saliency(fr, **kw).cpu().numpy()}
    for k in ('census', 'profile'):
        if k in kw:
            out[k] = kw[k].cpu().numpy()
    plan = ops.net_plan(h, w)
    last = n - (n - 1) // 32 * 32
    for name, div, ch in NET_TAPS:
        shape = (plan['NH'] // div, plan['NW'] // div, ch) if div else (h, w)
        out[name] = np.stack([eng.tap(getattr(ops, 'TAP_' + name), i, shape) for i in range(last)])
    return out


@pytest.mark.parametrize('h, w', NET_SHAPES)
@pytest.mark.parametrize('front', ['1', '0'])
@pytest.mark.parametrize('pipe', ['bf16x6', 'f32'])
def test_network_on_filled_and_on_dirty_scratch_equals_a_fresh_handle(net_engines, pipe, front, h, w):
    """Maps, census and profile rows and the taps FEAT4X .. PRE of every entry, under the three settings, straight and after a decoy
    (more frames of another geometry and other content: the workspace is larger and dirtier than the case needs), equal those of a
    handle created for the case."""
    dut = net_engines(pipe, front)
    for n in NET_COUNTS.get((h, w), (1, 3)):
        rng = np.random.RandomState(1000 * h + w + n)
        fr = torch.from_numpy(rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)).cuda()
        decoy = torch.from_numpy(rng.randint(0, 256, (n + 2,) + DECOY_SHAPE + (3,)).astype(np.uint8)).cuda()
        for entry in ENTRIES:
            ops.scratch_fill(None)
            fresh = _net_engine(pipe, front)
            try:
                want = _run_entry(fresh, fr, entry)
            finally:
                fresh.close()
            for setting in WS_SETTINGS:
                ops.scratch_fill(setting)
                for dirty in (False, True):
                    if dirty:
                        dut.saliency(decoy)
                    got = _run_entry(dut, fr, entry)
                    assert got.keys() == want.keys()
                    for k in want:
                        assert same(got[k], want[k]), (pipe, front, (h, w), n, entry, setting, dirty, k)


# ---- TransNet ---------------------------------------------------------------------------------------------------------------
SHOT_T = (1, 9, 17, 37, 100)


def _row_ranges(T):
    return [None] + [r for t, r in KEPT if t == T] + ([(10, 11)] if T >= 11 else [])


SHOT_CASES = [(T, rows) for T in SHOT_T for rows in _row_ranges(T)]


@functools.lru_cache(maxsize=None)
def _shot_sd():
    return R.variant_state_dict('seed0')


@pytest.fixture(scope='module')
def shot_nets():
    """Per pipe two networks on handles of their own: the one under test and the one that only ever runs the reference full passes."""
    made = {}

    def get(pipe):
        if pipe not in made:
            made[pipe] = (make_net(pipe, _shot_sd()), make_net(pipe, _shot_sd()))
        return made[pipe]
    yield get
    for a, b in made.values():
        a.close()
        b.close()


def _windows(nw, T, seed):
    return np.stack([R.frames(R.INPUTS[(seed + j) % len(R.INPUTS)], T, 7000 + 10 * seed + j) for j in range(nw)])


class _AfterDecoy:
    """The tap door of a network, each tap's pass behind a full pass over other windows of the same length and count."""

    def __init__(self, net, decoy):
        self.net, self.decoy = net, decoy

    def debug_tap(self, fr, layer, rows=None):
        self.net.predict_raw_device(self.decoy)
        return self.net.debug_tap(fr, layer, rows)


@pytest.mark.parametrize('T, rows', SHOT_CASES, ids=['T%d-%s' % (T, 'full' if r is None else '%d_%d' % r) for T, r in SHOT_CASES])
@pytest.mark.parametrize('pipe', list(PIPES))
def test_transnet_pass_after_a_decoy_full_pass_over_other_windows(shot_nets, pipe, T, rows):
    """The order is the point: a full pass over OTHER windows of the same T and count (same plane strides, same addresses), then the
    pass under test.  Its kept rows are bit for bit those of a full pass made on another handle, under the three settings, for 1 and 3
    windows; and every tap on the frames it computes is inside GATES of the float64 oracle and the same bits under the three settings."""
    dut, other = shot_nets(pipe)
    a, b = (0, T) if rows is None else rows
    for nw in (1, 3):
        fr = torch.from_numpy(_windows(nw, T, 3 * T + nw)).cuda()
        decoy = torch.from_numpy(_windows(nw, T, 3 * T + nw + 50)).cuda()
        ops.scratch_fill(None)
        want = other.predict_raw_device(fr).cpu().numpy()
        for setting in WS_SETTINGS:
            ops.scratch_fill(setting)
            dut.predict_raw_device(decoy)
            got = dut.predict_raw_device(fr, rows=rows).cpu().numpy()
            assert same(got[:, a:b], want[:, a:b]), (pipe, T, rows, nw, setting)
    sd, refs = shot_oracle('seed0')
    for fr, label, ref in refs:
        if fr.shape[1] != T:
            continue
        decoy = torch.from_numpy(_windows(fr.shape[0], T, 3 * T + 90)).cuda()
        frames_of = lambda layer: computed_frames(layer, T, a, b)
        taps = {}
        for setting in WS_SETTINGS:
            ops.scratch_fill(setting)
            door = _AfterDecoy(dut, decoy)
            if setting == WS_FILL:
                taps[setting] = check_layers(door, sd, pipe, fr, ref, '%s rows %s' % (label, rows), rows=rows, frames_of=frames_of)
            else:
                taps[setting] = {layer: door.debug_tap(fr, li, rows) for li, layer in enumerate(LAYERS)}
        for layer in LAYERS:
            s = frames_of(layer)
            for setting in WS_SETTINGS:
                assert same(taps[setting][layer][:, s], taps[WS_FILL][layer][:, s]), (pipe, label, rows, layer, setting)


def test_transnet_more_windows_than_one_pass_holds(shot_nets):
    """17 windows of 100 frames: the second pass over the workspace holds 2 windows where the first held 15.  Kept rows after a decoy
    full call over 17 other windows, against a full call on another handle."""
    dut, other = shot_nets('default')
    fr = torch.from_numpy(_windows(17, 100, 1)).cuda()
    decoy = torch.from_numpy(_windows(17, 100, 2)).cuda()
    ops.scratch_fill(None)
    want = other.predict_raw_device(fr).cpu().numpy()
    for setting in WS_SETTINGS:
        ops.scratch_fill(setting)
        dut.predict_raw_device(decoy)
        got = dut.predict_raw_device(fr, rows=(25, 75)).cpu().numpy()
        assert same(got[:, 25:75], want[:, 25:75]), setting
        dut.predict_raw_device(decoy)
        assert same(dut.predict_raw_device(fr).cpu().numpy(), want), setting


# ---- the tail, by history ---------------------------------------------------------------------------------------------------
DEFAULT, BEST = P.init_crop_params(), P.init_crop_params(True)
TAIL_X = {                                          # name: (parameter set, clust_filt, resize_factor, map shape)
    'default-35x62': (DEFAULT, True, 1, (35, 62)),
    'default-140x250': (DEFAULT, True, 1, (140, 250)),
    'default-f4-140x250': (DEFAULT, True, 4, (140, 250)),
    'default-nofilt-140x250': (DEFAULT, False, 1, (140, 250)),
    'best-140x250': (BEST, True, 4, (140, 250)),
    'best-f1-35x62': (BEST, True, 1, (35, 62)),
    'best-nofilt-140x250': (BEST, False, 4, (140, 250)),
    'best-nofilt-f1-35x62': (BEST, False, 1, (35, 62)),
}
TAIL_D = ('more', 'larger_shape', 'other_factor', 'longer_chain', 'other_form')
X_FLAGS = np.array([1, 1, 0, 0], np.uint8)          # a chain 0 -> 1 -> 2, map 3 alone


def blob_maps(n, h, w, cell, grid, seed):
    """n raw maps of h x w: one soft blob (peak 200 .. 255, above both thresholds within about 0.8 of its radius) per cell of a
    grid[0] x grid[1] grid, radius 4.5 * cell, jittered by the seed and the map's index, plus a few single pixels."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        m = np.zeros((h, w))
        for gy in range(grid[0]):
            for gx in range(grid[1]):
                cy = (gy + 0.5) * h / grid[0] + rng.uniform(-1, 1) * cell
                cx = (gx + 0.5) * w / grid[1] + rng.uniform(-1, 1) * cell
                r = 4.5 * cell * rng.uniform(0.85, 1.0)
                m = np.maximum(m, rng.uniform(200, 255) * np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (r * r)))
        m = m.astype(np.uint8)
        m[rng.rand(h, w) < 0.002] = 180
        out.append(m)
    return np.stack(out)


def _cp(name):
    base, filt, f, shape = TAIL_X[name]
    return dict(base, clust_filt=filt, resize_factor=f), shape


@functools.lru_cache(maxsize=None)
def tail_x(name):
    """Case X and what the oracle makes of it -> (CP, raw maps, (final maps, dx, dy), what the cluster filter saw of every map)."""
    CP, (h, w) = _cp(name)
    f = CP['resize_factor']
    maps = blob_maps(4, h, w, f if CP['clust_filt'] else 1, (2, 2), 31 + h + f)      # (blobs of the size the tail clusters at)
    final, dx, dy, _ = _ref_tail(maps, X_FLAGS, CP)
    thr = T.threshold(maps.copy(), CP['t_threshold'])
    seen = []
    for i in range(len(maps)):
        m = T.blend_next(final[i - 1], thr[i]) if i and X_FLAGS[i - 1] else thr[i]
        seen.append(cv_ref.resize_linear_factor_u8(m, 1.0 / f) if f > 1 and CP['clust_filt'] else m)
    return CP, maps, (final, dx, dy), seen


def tail_d(name, kind):
    """The decoy of case X: always more blobs, so more points and more clusters than X, and larger in the one way `kind` names
    -> (CP, raw maps, flags)."""
    CP, (h, w) = _cp(name)
    f = CP['resize_factor'] if CP['clust_filt'] else 1          # the factor of the shape X's tail works on
    CP = dict(CP, clust_filt=True, resize_factor=f)
    n, flags, cell = 4, X_FLAGS, f
    if kind == 'larger_shape':
        h, w = (70, 124) if (h, w) == (35, 62) else (200, 250)
    elif kind == 'other_factor':
        if f == 1:                                  # through the shrunk maps, which X never touches (a full map is 255 x 255 at most)
            CP, cell = dict(CP, resize_factor=4), 4
            if 4 * h <= 255 and 4 * w <= 255:
                h, w = 4 * h, 4 * w
        else:                                       # the full map clustered: sixteen times the points
            CP = dict(CP, resize_factor=1)
    elif kind == 'longer_chain':
        n, flags = 8, np.array([1] * 7 + [0], np.uint8)
    return CP, blob_maps(n, h, w, cell, (3, 4), 77 + h + len(kind)), flags


STATE_WORDS = (ops.HDR_NSEL, ops.HDR_KEPT, ops.HDR_NCLUSTERS)      # of a clustered map (N and CLUSTERED: of every map)


def _run_tail(eng, maps, flags, CP):
    dm = torch.from_numpy(maps.copy()).cuda()
    eng.threshold_(dm, CP['t_threshold'])
    xy, stats = eng.cluster_center_(dm, flags, CP, want_stats=True)
    states = [eng.cluster_state(i, maps[0].size) for i in range(len(maps))]
    return dm.cpu().numpy(), xy.cpu().numpy(), stats.cpu().numpy(), states


def _same_tail(a, b, where):
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2]), where
    for i, (s, t) in enumerate(zip(a[3], b[3])):
        assert s['n'] == t['n'] and same(s['pts'], t['pts']), (where, i)
        assert s['hdr'][ops.HDR_N] == t['hdr'][ops.HDR_N] and s['hdr'][ops.HDR_CLUSTERED] == t['hdr'][ops.HDR_CLUSTERED], (where, i)
        if s['hdr'][ops.HDR_CLUSTERED]:
            assert all(s['hdr'][k] == t['hdr'][k] for k in STATE_WORDS), (where, i, s['hdr'], t['hdr'])
            assert same(s['core'], t['core']) and same(s['mst'], t['mst']) and same(s['labels'], t['labels']), (where, i)


@pytest.mark.parametrize('kind', TAIL_D)
@pytest.mark.parametrize('name', list(TAIL_X))
def test_tail_after_a_larger_call_equals_a_fresh_handle_and_the_oracle(name, kind):
    """svc_cluster_center on X on a fresh handle and on a handle whose previous call was the decoy D, with the switch off (the history
    is what the second call starts on) and on: maps, centres, stats and svc_debug_cluster_state are the same either way and the
    oracle's.  D has more points and more condensed clusters than X on its largest map (read through svc_debug_cluster_state), or the
    decoy was none.  other_form: both handles with the one-node-per-step Prim and the serial hierarchy (SVC_PRIM_LVL / SVC_TREE_PAR 0),
    whose kernels keep in the workspace what the default form keeps on chip."""
    CP, maps, (final, dx, dy), seen = tail_x(name)
    dCP, dmaps, dflags = tail_d(name, kind)
    make = lambda: ops.tail_engine(reference=(kind == 'other_form'))
    ops.scratch_fill(None)
    fresh = make()
    try:
        want = _run_tail(fresh, maps, X_FLAGS, CP)
        assert np.array_equal(want[0], final), name
        for i in range(len(maps)):
            assert (dx[i] is None and np.isnan(want[1][i]).all()) or (want[1][i, 0] == dx[i] and want[1][i, 1] == dy[i]), (name, i)
            if CP['clust_filt']:
                _state_is_the_oracles(fresh, i, seen[i], CP)
    finally:
        fresh.close()
    for setting in (None, WS_FILL):
        ops.scratch_fill(setting)
        dut = make()
        try:
            d = _run_tail(dut, dmaps, dflags, dCP)
            got = _run_tail(dut, maps, X_FLAGS, CP)
        finally:
            dut.close()
        hx, hd = [s['hdr'] for s in want[3]], [s['hdr'] for s in d[3]]
        assert max(h[ops.HDR_N] for h in hd) > max(h[ops.HDR_N] for h in hx), (name, kind)
        if CP['clust_filt']:
            assert all(h[ops.HDR_CLUSTERED] for h in hd)
            assert max(h[ops.HDR_NCLUSTERS] for h in hd) > max(h[ops.HDR_NCLUSTERS] for h in hx if h[ops.HDR_CLUSTERED]), (name, kind)
        _same_tail(got, want, (name, kind, setting))


# ---- the switch itself ------------------------------------------------------------------------------------------------------
def test_the_fill_reaches_the_buffer_and_leaves_the_computed_frames_alone(shot_nets):
    """A pass for the kept rows 40 .. 49 computes cell 2 on the frames 8 .. 81.  With the switch on, its tap reads the fill (all ones:
    NaN in every bf16 plane) on the first and the last frame of the window, and the computed frames hold the bits they hold with the
    switch off.  Channels 16 .. 63 only: the planes of the first 16 channels start where the pass has put its input planes (24 bytes
    per position; a tile of 16 channels takes 96), the others lie behind everything the pass wrote before cell 2."""
    dut, _ = shot_nets('default')
    fr = torch.from_numpy(_windows(1, 100, 5)).cuda()
    li = LAYERS.index('cell2')
    s = computed_frames('cell2', 100, 40, 50)
    assert (s.start, s.stop) == (8, 82)
    ops.scratch_fill(None)
    plain = dut.debug_tap(fr, li, (40, 50))
    ops.scratch_fill(WS_FILL)
    filled = dut.debug_tap(fr, li, (40, 50))
    assert np.isnan(filled[:, 0, :, :, 16:]).all() and np.isnan(filled[:, 99, :, :, 16:]).all()
    assert same(filled[:, s], plain[:, s]) and np.isfinite(plain[:, s]).all()


def test_the_switch_off_changes_nothing_and_refuses_what_is_no_byte(engine, shot_nets):
    """The bytes of a plain pass of each part with the switch off equal those with it on; off is what a process starts with and what
    the fixture leaves; -2 and 256 are refused and leave the switch as it was."""
    dut, _ = shot_nets('default')
    rng = np.random.RandomState(9)
    fr = torch.from_numpy(rng.randint(0, 256, (3, 140, 250, 3)).astype(np.uint8)).cuda()
    win = torch.from_numpy(_windows(2, 37, 8)).cuda()
    maps = blob_maps(4, 140, 250, 4, (2, 2), 5)
    got = {}
    for setting in WS_SETTINGS:
        ops.scratch_fill(setting)
        for bad in (-2, 256):
            with pytest.raises(SvcError, match='svc_debug_scratch_fill'):
                ops.scratch_fill(bad)
        tail = _run_tail(engine, maps, X_FLAGS, BEST)
        got[setting] = (engine.saliency(fr).cpu().numpy(), dut.predict_raw_device(win).cpu().numpy()) + tail[:3]
    for setting in WS_SETTINGS[1:]:
        for a, b in zip(got[setting], got[None]):
            assert same(a, b), setting
