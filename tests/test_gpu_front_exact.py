"""-m gpu: k_front (LANCZOS + normalisation + features.0 + features.1 in one kernel) against the three kernels it replaces
(SVC_FRONT=0), bit for bit, at every geometry that runs it.

k_front walks its vertical pass with a register window and scalar coefficient records, takes its column tables from the plan
and leaves out the features.0 MFMA whose two taps are both padding; the three kernels do none of that.  So equality here shows
that the window, the records, the clamps and the dropped + 0 product change nothing: the normalised network input (the
integer resampling and the LUT), an fp32 feature tap behind features.1, and the maps.

Frames per geometry: random bytes, all 0, all 255, a one-pixel checkerboard of 0 and 255 (LANCZOS over- and undershoots, so
both passes hit both clamps), and a frame whose first and last rows and columns differ from the interior (window start, end
rows, zero padding).  n = 3 frames: the grid is then no multiple of 8 at most geometries, so the XCD-ordered block index meets
a ragged last round."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import unisal_ref as U
from retargetvid_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

# one saliency-map shape per network input size get_optimal_out_size can select; all eleven up-scale, so all run k_front
_SHAPES = [(140, 250), (187, 250), (250, 140), (166, 250), (200, 250), (230, 250), (249, 249), (250, 230), (250, 200),
           (250, 187), (250, 166)]


def _engine_with(sd, **env):
    """An engine created under the given environment (the knobs are read when the handle is created)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ops.Engine(sd)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def three_kernels(synthetic_sd):
    eng = _engine_with(synthetic_sd, SVC_FRONT='0')
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def fused_no_tap(synthetic_sd):
    """The default outside the tests: k_front without the write of the network input."""
    eng = _engine_with(synthetic_sd, SVC_KEEP_INPUT='0')
    yield eng
    eng.close()


def _frames(h, w):
    """name -> [3][h][w][3] u8"""
    rng = np.random.RandomState(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    checker = np.stack([np.repeat(b[:, :, None], 3, 2) for b in (board, 255 - board, board)])
    checker[2, :, :, 1] = 255 - board                              # the channels out of phase
    edge = np.empty((3, h, w, 3), np.uint8)
    for i, (inner, rim) in enumerate(((128, 0), (0, 255), (255, 1))):
        edge[i] = inner
        edge[i, 0], edge[i, -1], edge[i, :, 0], edge[i, :, -1] = rim, 255 - rim, rim // 2 + 3, 255 - rim // 2
    return {'random': rng.randint(0, 256, (3, h, w, 3)).astype(np.uint8),
            'zeros': np.zeros((3, h, w, 3), np.uint8),
            'full': np.full((3, h, w, 3), 255, np.uint8),
            'checker': checker,
            'edge': edge}


@pytest.mark.parametrize('shape', _SHAPES)
def test_front_kernel_equals_the_three_kernels_on_extreme_frames(engine, three_kernels, fused_no_tap, shape):
    h, w = shape
    NH, NW = U.get_optimal_out_size((h, w))
    assert h <= NH and w <= NW
    for name, fr in _frames(h, w).items():
        dev = torch.from_numpy(fr).cuda()
        ref_maps = three_kernels.saliency(dev).cpu().numpy()
        assert not three_kernels.front_fused()
        ref_in = [three_kernels.tap(ops.TAP_INPUT, i, (NH, NW, 3)) for i in range(3)]
        ref_f4 = [three_kernels.tap(ops.TAP_FEAT4X, i, (NH // 8, NW // 8, 64)) for i in range(3)]
        if name == 'checker':                                       # the frame is there to reach both clamps: see that it does
            lo, hi = ref_in[0][:, :, 0].min(), ref_in[0][:, :, 0].max()
            assert lo == np.float32((np.float32(0) / np.float32(255) - np.float32(0.485)) / np.float32(0.229))
            assert hi == np.float32((np.float32(255) / np.float32(255) - np.float32(0.485)) / np.float32(0.229))
        maps = engine.saliency(dev).cpu().numpy()                   # SVC_KEEP_INPUT=1 (tests/conftest.py): k_front writes the input tap
        assert engine.front_fused()
        assert np.array_equal(maps, ref_maps), (shape, name)
        for i in range(3):
            assert np.array_equal(engine.tap(ops.TAP_INPUT, i, (NH, NW, 3)), ref_in[i]), (shape, name, i)
            assert np.array_equal(engine.tap(ops.TAP_FEAT4X, i, (NH // 8, NW // 8, 64)), ref_f4[i]), (shape, name, i)
        maps = fused_no_tap.saliency(dev).cpu().numpy()             # default settings
        assert fused_no_tap.front_fused()
        assert np.array_equal(maps, ref_maps), (shape, name)
        for i in range(3):
            assert np.array_equal(fused_no_tap.tap(ops.TAP_FEAT4X, i, (NH // 8, NW // 8, 64)), ref_f4[i]), (shape, name, i)
