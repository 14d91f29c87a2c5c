"""-m gpu: k_dwpw's halo taps at the edges of the image and of the input buffer, bit for bit against the float64 node oracle.

The kernel reads its 18 taps per lane through a buffer resource that spans ONE frame, by 32-bit byte offsets: a tap outside the
image reads 0 because its offset is not below the resource's size (a row above the image, a column beside it: an offset of 2^31;
a row below it likewise), not because anything selects a zero.  What can go wrong with that, and what the exact cases of
tests/test_gpu_net_nodes.py (n = 3 and 4, uniform grid inputs) do not direct:

  * n = 1 and n = 2: the frame under test is the first AND the last of its buffer.  A tap above row 0 of frame 0 lies below the
    buffer; a tap below the last row of the last frame lies in the NaN fill behind the n frames (svc_debug_run_node's fill for a
    node input, the scratch fill for an intermediate).
  * one node per column-tile count NT and per level: block9 (NT 2, H/16), block12 (NT 3), block14 (NT 5, 8-wide patches), block16
    (NT 5, the lowest level: 16-wide patches where it is 13 or 10 wide), post_cnn (NT 4, C = 1296: the short last chunk), post_us2
    (NT 2, the largest level, H/8).
  * two geometries: '16x9', whose 8x13 and 16x26 levels put the right border inside a tile, and '1x1', the smallest of the eleven
    by network pixels (40x40, 20x20, 10x10).
  * border-heavy inputs: the dyadic grid of the exact cases, the two outermost rows and columns of every frame set to the grid's
    extremes.  A tap that wraps into the neighbouring row, or comes from the neighbouring frame, then changes the depthwise sum
    by a large amount.  A NaN tap would not survive the ReLU6 (fmaxf(NaN, 0) = 0), so the assertion is the exact comparison."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import net_node_cases as C
from oracle import unisal_nodes_ref as N
from test_gpu_net_nodes import PIPES, _assert_rest_is_fill, _engine
from test_oracle_unisal import ELEVEN, NET_SIZES

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

NODES = ('block9', 'block12', 'block14', 'block16', 'post_cnn', 'post_us2')
GEOMS = ('16x9', '1x1')
assert GEOMS[1] == min(NET_SIZES, key=lambda g: NET_SIZES[g][0] * NET_SIZES[g][1])
CASES = [(g, n) for g in GEOMS for n in (1, 2)]


def border_inputs(node, n, NH, NW, seed):
    """exact_inputs, with the two outermost rows and columns of every frame at the extremes of the input's grid (either, at random)."""
    rng = np.random.RandomState(seed + 7)
    out = []
    for a in C.exact_inputs(node, n, NH, NW, seed):
        if a is not None:
            H, W = a.shape[1:3]
            edge = np.zeros((H, W), bool)
            edge[:2], edge[-2:], edge[:, :2], edge[:, -2:] = True, True, True, True
            grid = np.unique(a)
            lo, hi = grid[0], grid[-1]
            assert lo == -4.0 and hi in (3.5, 3.875)
            a[:, edge] = rng.choice(np.array([lo, hi], np.float32), (n, int(edge.sum())) + a.shape[3:])
        out.append(a)
    return out


@pytest.fixture(scope='module')
def exact_engines():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    made = {pipe: _engine(pipe, layers=C.exact_layers()) for pipe in PIPES}
    yield made
    for e in made.values():
        e.close()


@pytest.mark.parametrize('gname,n', CASES)
def test_border_taps_equal_the_float64_value_bit_for_bit(exact_engines, gname, n):
    h, w = ELEVEN[gname]
    NH, NW = NET_SIZES[gname]
    layers = C.exact_layers()
    for i, node in enumerate(NODES):
        ref = N.NodeRef(layers, bounds=False, track=True)
        in0, in1 = border_inputs(node, n, NH, NW, seed=1000 * n + 31 * i + NH)
        value, _ = ref.run(node, in0, in1)
        ok, worst = C.budget_ok(ref)
        assert ok, (node, 'a partial sum may not be an fp32 number', worst)
        for pipe in PIPES:
            where = (gname, n, node, pipe)
            dev, rest = C.run_device(exact_engines[pipe], node, n, h, w, NH, NW, in0, in1)
            assert not np.isnan(dev).any(), (where, 'unwritten elements', int(np.isnan(dev).sum()), np.argwhere(np.isnan(dev))[:4].tolist())
            bad = dev.astype(np.float64) != value
            assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(dev - value).max()))
            _assert_rest_is_fill(rest, where)
