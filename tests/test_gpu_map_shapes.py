"""-m gpu: the three kernels whose work depends on the saliency-map shape (h, w) itself -- k_front and k_lanczos_norm (Pillow
LANCZOS (h, w) -> (NH, NW)) and k_smooth_down_mfma (smoothing + bilinear (NH, NW) -> (h, w)) -- at the shapes of
tests/test_net_plan_census.py: SHAPES, each there for an extreme of the plan's geometry over every shape the ingest can produce
(realistic ratios outside the eleven, narrow maps, wide strips where the smoothing kernel takes fewer rows per band, the
smallest map, axes that are not resampled), and the down-scaling frames of the three-kernel path.

Per shape, three frames (blobs, random bytes, the rim frame of tests/test_gpu_front_exact.py) on the carrier checkpoint, both
matrix pipes.  No tolerance is made here: the network input equals the oracle's bit for bit; k_front equals the three kernels bit
for bit; the front and smooth nodes are held to net_node_cases.gate_c against the float64 node oracle; the u8 maps to the gate of
tests/test_gpu_geometries.py (one grey level on less than the _TOL fraction of the pixels)."""
import functools
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import net_node_cases as C
from oracle import unisal_nodes_ref as N, unisal_ref as U
from retargetvid_amd import _lib, ops, synth, weights
from test_gpu_front_exact import _engine_with, _frames, three_kernels  # noqa: F401  (three_kernels: a fixture)
from test_gpu_net_nodes import PIPES, _assert_rest_is_fill, _engine, _gate
from test_gpu_parity import _TOL
from test_net_plan_census import DOWN_SHAPES, REFUSED, SD_ROWS, SHAPES

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

IDENTITY = [(416, 256), (416, 250)]                     # saliency entry only: the tail takes maps of at most 255 a side
NODE_SHAPES = [s for s in SHAPES if s not in IDENTITY]
U8_FRAC = _TOL['nc'][2]                                 # the carrier checkpoint's gate (tests/test_gpu_geometries.py: GATES)
U8_MIN_PX = 20000                                       # below it a fraction of the pixels is one or two pixels: the node checks hold those shapes
_id = lambda s: '%dx%d' % s


@pytest.fixture(scope='module')
def pipes(synthetic_sd):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    engs = {pipe: _engine(pipe, sd=synthetic_sd) for pipe in PIPES}
    yield engs
    for e in engs.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _node_ref():
    sd = weights.make_synthetic_state_dict(0)
    return sd, N.NodeRef(weights.fold_state_dict(sd), sd['smoothing_salicon.weight'])


def _shape_frames(h, w, n=3):
    rng = np.random.RandomState(7 * h + w)
    fr = np.stack([synth.blob_frames(1, h, w, seed=3 * h + w)[0], rng.randint(0, 256, (h, w, 3)).astype(np.uint8), _frames(h, w)['edge'][2]])
    return np.ascontiguousarray(fr[:n])


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """Computed once per shape and shared, never written to: frames, the fp32 oracle's network input, u8 maps and adapt output."""
    h, w = shape
    fr = _shape_frames(h, w)
    taps = {}
    maps = np.transpose(U.saliency_u8(_node_ref()[0], fr, taps), (2, 0, 1))
    adapt = np.stack([t['adapt'][0].numpy() for t in taps['frames']])
    out = dict(frames=fr, input=C.network_input(fr, torch.float32), maps=maps, adapt=adapt)
    for v in out.values():
        v.setflags(write=False)
    return out


def _taps(eng, which, n, shape):
    return np.stack([eng.tap(which, i, shape) for i in range(n)])


def _logit_fields(adapt, H3, W3):
    """name -> [3, H3, W3]: the oracle's own adapt output; N(0, 1); a checkerboard of cells plus a ramp in y, so that every 8 x 8
    cell of the network-size map differs from each neighbour by at least 1 -- a band that reads a network row it did not stage,
    or a row one off, is then wrong by far more than rounding."""
    rng = np.random.RandomState(H3 * 100 + W3)
    yy, xx = np.mgrid[0:H3, 0:W3]
    board = np.stack([3.0 * ((yy + xx + i) & 1) + 1.0 * yy - 0.5 * i for i in range(3)])
    assert (np.abs(np.diff(board, axis=1)) >= 1).all() and (np.abs(np.diff(board, axis=2)) >= 1).all()
    return {'adapt': adapt.astype(np.float32), 'normal': rng.standard_normal((3, H3, W3)).astype(np.float32), 'cells': board.astype(np.float32)}


# ---- input and front ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES), ids=_id)
def test_network_input_is_the_oracles_and_k_front_equals_the_three_kernels(pipes, three_kernels, shape):
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    o = _oracle(shape)
    dev = torch.tensor(o['frames']).cuda()
    for pipe, eng in pipes.items():
        maps = eng.saliency(dev).cpu().numpy()
        assert eng.front_fused(), (shape, pipe)
        got = _taps(eng, ops.TAP_INPUT, 3, (NH, NW, 3))
        assert np.array_equal(got.view(np.uint32), o['input'].view(np.uint32)), (shape, pipe, np.argwhere(got != o['input'])[:4].tolist())
        if pipe == 'bf16x6':                                        # the pipe of the three-kernel handle (the default)
            f4 = _taps(eng, ops.TAP_FEAT4X, 3, (NH // 8, NW // 8, 64))
            ref_maps = three_kernels.saliency(dev).cpu().numpy()
            assert not three_kernels.front_fused() and three_kernels.matrix_pipe() == pipe
            assert np.array_equal(_taps(three_kernels, ops.TAP_INPUT, 3, (NH, NW, 3)).view(np.uint32), got.view(np.uint32)), shape
            assert np.array_equal(_taps(three_kernels, ops.TAP_FEAT4X, 3, (NH // 8, NW // 8, 64)).view(np.uint32), f4.view(np.uint32)), shape
            assert np.array_equal(maps, ref_maps), shape


@pytest.mark.parametrize('shape', NODE_SHAPES, ids=_id)
def test_front_node_within_its_gate(pipes, shape):
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    o = _oracle(shape)
    value, bound = _node_ref()[1].run('front', o['input'])
    for pipe, eng in pipes.items():
        dev, _ = C.run_device(eng, 'front', 3, h, w, NH, NW, o['frames'])
        print(shape, pipe, 'front ratio %.4f of %.4f' % (C.error_ratio(dev, value, bound), C.gate_c('front')))
        _gate(dev, value, bound, C.gate_c('front'), (shape, 'front', pipe))


# ---- last stage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['adapt', 'normal', 'cells'])
@pytest.mark.parametrize('shape', NODE_SHAPES, ids=_id)
def test_smooth_node_within_its_gate_on_three_logit_fields(pipes, shape, name):
    """The output is pre-filled with NaN by the door: _gate's finiteness check is the check that every pixel of every band was
    written.  64x250 keeps SD_ROWS rows per band, 63x250 is the first strip with fewer: both are in the table.  (One case per
    field: the float64 41 x 41 convolutions of the reference are what a case costs.)"""
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    logit = _logit_fields(_oracle(shape)['adapt'], NH // 8, NW // 8)[name]
    value, bound = _node_ref()[1].run('smooth', logit, out_hw=(h, w))
    for pipe, eng in pipes.items():
        where = (shape, 'smooth', name, pipe)
        dev, rest = C.run_device(eng, 'smooth', 3, h, w, NH, NW, logit)
        assert dev.shape == (3, h, w), where
        print(where, 'ratio %.3f of %.3f' % (C.error_ratio(dev, value, bound), C.gate_c('smooth')))
        _gate(dev, value, bound, C.gate_c('smooth'), where)
        _assert_rest_is_fill(rest, where)


# ---- whole pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES), ids=_id)
def test_whole_pass_finite_batch_independent_and_within_a_grey_level_of_the_oracle(pipes, shape):
    h, w = shape
    o = _oracle(shape)
    dev = torch.tensor(o['frames']).cuda()
    for pipe, eng in pipes.items():
        maps = eng.saliency(dev)
        assert tuple(maps.shape) == (3, h, w) and maps.dtype == torch.uint8, (shape, pipe)
        pre = _taps(eng, ops.TAP_PRE, 3, (h, w))
        assert np.isfinite(pre).all(), (shape, pipe)
        assert int(maps.amax()) == 255, (shape, pipe)               # the map's maximum is 255 by construction: exp(0) * 255
        assert torch.equal(eng.saliency(dev[1:2])[0], maps[1]), (shape, pipe, 'a frame alone')
        if h * w >= U8_MIN_PX:
            m = maps.cpu().numpy()
            for i in range(3):
                du = np.abs(m[i].astype(int) - o['maps'][i].astype(int))
                print(shape, pipe, i, 'u8 max %d fraction %.2e' % (du.max(), (du > 0).mean()))
                assert du.max() <= 1 and (du > 0).mean() < U8_FRAC, (shape, pipe, i, int(du.max()), float((du > 0).mean()))


@pytest.mark.parametrize('shape', [(104, 250), (250, 35), (19, 250)], ids=_id)
def test_the_door_walks_what_the_pass_runs_from_the_last_decoder_block_on(pipes, shape):
    """Section (c) of tests/test_gpu_net_nodes.py from post_us2 on: adapt and smooth through the door on the pass's own DEC tap
    end in the bytes of its PRE tap -- the door plans these shapes as the pass does."""
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    eng = pipes['bf16x6']
    eng.saliency(torch.tensor(_oracle(shape)['frames']).cuda())
    dec = _taps(eng, ops.TAP_DEC, 3, (NH // 8, NW // 8, 64))
    pre = _taps(eng, ops.TAP_PRE, 3, (h, w))
    run = lambda node, a: C.run_device(eng, node, 3, h, w, NH, NW, a)[0]
    got = run('smooth', run('adapt', dec))
    assert np.array_equal(got.view(np.uint32), pre.view(np.uint32)), shape


# ---- rows per band ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(140, 250), (104, 250)], ids=_id)
def test_one_row_per_band_gives_the_bytes_of_the_default(engine, synthetic_sd, shape):
    """A pixel of the smoothing kernel comes from its own cell's MFMA chain and its own four tile values, so the map cannot depend on
    the rows per band: a handle forced to one row per band (SVC_SD_ROWS=1) gives the default's PRE tap and maps bit for bit."""
    h, w = shape
    assert ops.net_plan(h, w)['sd_rows'] == SD_ROWS
    dev = torch.from_numpy(_shape_frames(h, w)).cuda()
    maps = engine.saliency(dev)
    pre = _taps(engine, ops.TAP_PRE, 3, (h, w))
    one = _engine_with(synthetic_sd, SVC_SD_ROWS='1')
    try:
        assert torch.equal(one.saliency(dev), maps), shape
        assert np.array_equal(_taps(one, ops.TAP_PRE, 3, (h, w)).view(np.uint32), pre.view(np.uint32)), shape
    finally:
        one.close()


def test_the_rows_per_band_knob_is_checked(synthetic_sd):
    for bad in ('0', '8', 'x'):
        with pytest.raises(_lib.SvcError, match='SVC_SD_ROWS'):
            _engine_with(synthetic_sd, SVC_SD_ROWS=bad)


# ---- down-scaling frames: the three-kernel path -------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(DOWN_SHAPES), ids=_id)
def test_down_scaling_network_input_is_the_oracles(engine, shape):
    """k_lanczos_norm with nine taps and more (417x257: nine, out of k_front by one pixel; 540x960: the largest tile that fits in
    the CU's LDS) against the oracle's LANCZOS and normalisation, bit for bit."""
    h, w = shape
    NH, NW = U.get_optimal_out_size(shape)
    fr = _shape_frames(h, w, n=2)
    maps = engine.saliency(torch.from_numpy(fr).cuda())
    assert not engine.front_fused() and tuple(maps.shape) == (2, h, w), shape
    got = _taps(engine, ops.TAP_INPUT, 2, (NH, NW, 3))
    ref = C.network_input(fr, torch.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (shape, np.argwhere(got != ref)[:4].tolist())


def test_a_frame_over_the_lds_budget_is_refused_and_the_handle_serves_on(synthetic_sd):
    """720x1280 needs 226 272 B for a tile of k_lanczos_norm: refused in the plan with the frame size and the byte count, nothing
    launched, the maps untouched.  540x960 (143 616 B) runs.  The handle then gives a 140x250 call the bytes of a fresh handle."""
    (h, w), lds = next(iter(REFUSED.items()))
    assert (h, w, lds) == (720, 1280, 226272) and ops.net_plan(h, w)['lz_lds'] == lds
    fresh = ops.Engine(synthetic_sd)
    eng = ops.Engine(synthetic_sd)
    try:
        small = torch.from_numpy(_shape_frames(140, 250)).cuda()
        want = fresh.saliency(small)
        want_pre = _taps(fresh, ops.TAP_PRE, 3, (140, 250))
        eng.saliency(small[:1])                                     # a plan to keep
        big = torch.zeros((1, h, w, 3), dtype=torch.uint8, device='cuda')
        out = torch.full((1, h, w), 7, dtype=torch.uint8, device='cuda')
        for cls in ('lanczos', 'stem', 'smooth'):
            eng.profile_enable(cls)
            with pytest.raises(_lib.SvcError, match=r'720x1280 frame needs 226272 bytes of LDS.*svc_resize_frames_u8'):
                eng.saliency(big, out=out)
            assert eng.profile_read()[1] == 0, cls
        eng.profile_enable(None)
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        with pytest.raises(_lib.SvcError, match='1080x1920 frame needs 436768 bytes'):
            eng.saliency(torch.zeros((1, 1080, 1920, 3), dtype=torch.uint8, device='cuda'))
        mid = eng.saliency(torch.from_numpy(_shape_frames(540, 960, n=1)).cuda())
        assert tuple(mid.shape) == (1, 540, 960) and not eng.front_fused()
        assert torch.equal(eng.saliency(small), want)
        assert np.array_equal(_taps(eng, ops.TAP_PRE, 3, (140, 250)).view(np.uint32), want_pre.view(np.uint32))
    finally:
        eng.close()
        fresh.close()
