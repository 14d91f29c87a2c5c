"""-m gpu: the edge sort (k_sort) at every seam of its forms, and everything behind the MST on maps of up to 65 025 points, against
oracles that share no code with the device.

THE DOOR       every key array of tests/edge_order_cases.py through Engine.argsort_u32 (the routine k_sort runs) equals
               oracle/npsort_ref.py, which tests/test_edge_order_host.py pins to live numpy: every n from 1 to 70, the LDS / global
               seam (taken from the plan door, ops.sort_plan), 32 767 to 65 535 keys, keys above 2^31, and adversaries with up to 242
               heap-sorted ranges, ranges of 16 elements or fewer, ranges with ties, in LDS and in global memory.
THE SEAM       maps of cap + 1 and cap + 2 points in one call: k_sort's last LDS size and its first global one in production, against
               the full oracle.
LARGE MAPS     the six largest-geometry maps and a 20 000-point blob with holes, default and best-like parameters.  The exact Prim
               sequence above 22 000 points stays pinned to the one-node-per-step device Prim (tests/test_gpu_parity.py: the oracle's
               Prim is O(N^2) in Python); everything else is checked here: points, core distances (KD-tree), the edge list as a Prim
               walk with exact weights, the edge order, labels, cluster count, final map and centre -- the hierarchy by the oracle's
               back half run on the device's own MST.
Every comparison is equality."""
import time

import numpy as np
import pytest
import torch

import edge_order_cases as C
import tail_paths as tp
from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import hdbscan_ref as H, tail_ref as T
from retargetvid_amd import ops
from test_gpu_parity import _check_tail
from test_gpu_tail_paths import _state_is_the_oracles

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

PARAM_SETS = {'default': tp.DEFAULT, 'best_like': tp.BEST_LIKE}


def _door_equals_the_oracle(engine, label, keys):
    t0 = time.perf_counter()
    got = engine.argsort_u32(keys)
    dt = time.perf_counter() - t0
    want = C.expected_order(label, keys)
    form = 'LDS' if ops.sort_plan(len(keys))['in_lds'] else 'global'
    print('argsort_u32 %-28s n %5d %-6s %.1f ms' % (label, len(keys), form, 1e3 * dt))
    assert got.dtype == np.int32 and got.shape == want.shape
    if not np.array_equal(got, want):
        first = int(np.nonzero(got != want)[0][0])
        pytest.fail('%s, %d keys (%s form): the device order differs from numpy\'s at %d positions, first at %d (device %d, numpy %d)'
                    % (label, len(keys), form, int((got != want).sum()), first, got[first], want[first]))
    return dt


# ---- the door -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', C.FAMILIES)
def test_door_every_size_of_a_family(engine, family):
    """1 .. 70 keys (the first partition's children on either side of the 16 / 17 insertion-sort threshold), cap - 1 .. cap + 2
    (both sides of the LDS / global seam, cap from the plan door) and, for six families, 32 767 .. 65 535 keys (the 16-bit counters
    and indices with nothing to spare; 65 024 is a 255 x 255 map's edge count)."""
    cap = C.lds_cap()
    sizes = C.sizes_of(family, cap)
    assert [ops.sort_plan(n)['in_lds'] for n in (cap - 1, cap, cap + 1, cap + 2)] == [1, 1, 0, 0]
    for n in sizes:
        _door_equals_the_oracle(engine, (family, n), C.family_keys(family, n))


@pytest.mark.parametrize('label', C.ADVERSARY_LABELS)
def test_door_adversaries_reach_the_heapsort_fall_back(engine, label):
    """The depth limit in every way the device tells apart (tests/test_edge_order_host.py has the census): one heap-sorted range of
    about 6 000 elements in LDS and in global memory, 8 to 24 ranges per array in pairs of one depth (two threads of one step),
    ranges of 11 to 16 elements (heap-sorted although small enough for the insertion sort, as in numpy) -- all of distinct keys --
    and the coarse killers, whose 23 to 242 heap-sorted ranges hold ties: there the result depends on WHICH ranges the depth rule
    hands to the heapsort (a depth limit off by one, the other side pushed, size tested before depth all change it)."""
    keys = C.adversaries(C.lds_cap())[label]
    st = {}
    C.expected_order(label, keys, st)
    assert st['heapsorts'] >= 1
    dt = _door_equals_the_oracle(engine, label, keys)
    assert dt < 5.0, '%s took %.1f s on the device' % (label, dt)


def test_door_refuses_what_the_plan_door_refuses(engine):
    from retargetvid_amd._lib import SvcError
    for n in (0, C.MAX_KEYS + 1):
        with pytest.raises(SvcError):
            engine.argsort_u32(np.zeros(n, np.uint32))
        with pytest.raises(SvcError):
            ops.sort_plan(n)


# ---- the seam in production -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pname', list(PARAM_SETS))
def test_k_sort_at_the_lds_global_seam_in_one_call(engine, pname):
    """80 x 100 noise maps of cap + 1 and cap + 2 points in ONE call, without and with a blend flag: final maps and centres
    (_check_tail), point list, core distances, Prim edge list and labels (_state_is_the_oracles) are the full oracle's.  Without the
    flag the two maps have cap and cap + 1 edges: k_sort keeps the first in LDS and takes the second to global memory."""
    CP = PARAM_SETS[pname]
    cap = C.lds_cap()
    maps = C.seam_maps(cap)
    for flags in (None, np.array([1, 0], np.uint8)):
        seen, final, dx, dy = tp.blended_inputs(maps, flags, CP)
        _check_tail(engine, maps, flags, CP, (final, dx, dy, None))
        for i in range(2):
            st, o = _state_is_the_oracles(engine, i, seen[i], CP)
            assert o is not None and st['hdr'][ops.HDR_CLUSTERED] == 1
            assert st['hdr'][ops.HDR_NCLUSTERS] == o['nclusters'], i
            n_edges = st['n'] - 1
            order = engine.argsort_u32(st['mst'][:, 2])
            assert np.array_equal(order, C.expected_order(('seam', pname, flags is None, i), st['mst'][:, 2])), i
            print('seam map %d (%s, %s): %d edges, %s form, HDR_T_SORTED %d ticks'
                  % (i, pname, 'no flag' if flags is None else 'blended', n_edges, 'LDS' if ops.sort_plan(n_edges)['in_lds'] else 'global',
                     st['hdr'][ops.HDR_T_SORTED]))
            if flags is None:
                assert n_edges == cap + i and ops.sort_plan(n_edges)['in_lds'] == 1 - i


# ---- large maps: everything behind the MST ------------------------------------------------------------------------------------------
def _run_one(engine, m, CP):
    """One map through the tail -> (final map, centre [2], state)."""
    dm = torch.from_numpy(m[None].copy()).cuda()
    engine.threshold_(dm, CP['t_threshold'])
    xy = engine.cluster_center_(dm, None, CP)
    return dm.cpu().numpy()[0], xy.cpu().numpy()[0], engine.cluster_state(0, m.size)


@pytest.mark.parametrize('pname', list(PARAM_SETS))
@pytest.mark.parametrize('name', C.LARGE_MAP_NAMES)
def test_large_maps_behind_the_mst_are_the_oracles(engine, name, pname):
    CP = PARAM_SETS[pname]
    m = C.large_map(name)
    thr = T.threshold(m.copy(), CP['t_threshold'])
    got_map, got_xy, st = _run_one(engine, m, CP)
    hdr = st['hdr']
    # 1. the points
    X = np.argwhere(thr > 0).astype(np.int64)
    assert st['n'] == len(X) and np.array_equal(np.stack([st['pts'] & 255, (st['pts'] >> 8) & 255], 1), X)
    assert len(X) > 9500 and hdr[ops.HDR_CLUSTERED] == 1
    # 2. the core distances
    k = H.effective_min_samples(len(X), CP['hdbscan_min'], CP['hdbscan_min_samples'])
    core = C.kdtree_core(X, k)
    assert np.array_equal(st['core'], core)
    # 3. a spanning tree in Prim shape, every weight the minimum over the points visited before
    mst = st['mst'].astype(np.int64)
    assert C.mst_faults(X, core, mst) == []
    # 8. (the 20 000-point map) the Prim sequence itself
    if name == '140x250/holes':
        assert np.array_equal(np.stack(H.prim_mst(X, core), 1), mst)
    # 4. the device's own weights through the door
    order = C.expected_order(('large', name, pname), mst[:, 2])
    assert np.array_equal(engine.argsort_u32(st['mst'][:, 2]), order)
    # 5. 6. labels and cluster count: the oracle's back half on the device's MST
    labels, nclusters = C.back_half(mst, CP['hdbscan_min'], order)
    assert C.same_partition(labels, st['labels'])
    assert hdr[ops.HDR_NCLUSTERS] == nclusters
    plan = engine.tail_plan(m.shape[0], m.shape[1], CP)
    hier = tp.predict_hierarchy(len(X), nclusters, CP, plan)
    print('%s %s: N %d, %d condensed clusters (cap %d), hierarchy by %s, HDR_T_SORTED %d ticks'
          % (name, pname, len(X), nclusters, hier['cap'], 'k_tree_par' if hdr[ops.HDR_TREE_PAR] else 'k_tree', hdr[ops.HDR_T_SORTED]))
    assert hdr[ops.HDR_TREE_PAR] == hier['tree_par'] and hdr[ops.HDR_BACK_DONE] == hier['back_done']
    # 7. the final map and the centre, with those labels plugged into the oracle's filter
    final = T.clustering_filt(thr, CP, labels_fn=lambda X_, mcs, ms: labels)
    dx, dy = T.centers(np.ascontiguousarray(final[:, :, None]), CP)
    assert np.array_equal(got_map, final)
    if dx[0] is None:
        assert np.isnan(got_xy).all()
    else:
        assert got_xy[0] == dx[0] and got_xy[1] == dy[0]


def test_both_hierarchy_builders_take_large_maps(engine):
    """Which builder took each large map (HDR_TREE_PAR: 1 = k_tree_par kept it, 0 = handed to k_tree): both occur, so the cases
    above check both against the oracle."""
    took = {}
    for pname, CP in PARAM_SETS.items():
        for name in C.LARGE_MAP_NAMES:
            took[(name, pname)] = int(_run_one(engine, C.large_map(name), CP)[2]['hdr'][ops.HDR_TREE_PAR])
    print('HDR_TREE_PAR per large map:', took)
    assert set(took.values()) == {0, 1}
    assert {v for (n, p), v in took.items() if p == 'best_like'} == {0, 1}
