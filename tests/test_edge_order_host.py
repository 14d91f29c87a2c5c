"""The cases of tests/edge_order_cases.py lie where they are meant to lie, and their references are pinned (CPU only).

PIN     oracle/npsort_ref.py is pinned to numpy's scalar introsort by committed permutations (tests/golden/npsort_golden.npz).  Here
        it is pinned a second time, against the numpy that runs the tests: numpy's SIMD argsort covers 32- and 64-bit keys only, so
        np.argsort of uint16 keys takes the scalar routine on every CPU.  That call must first reproduce the committed goldens whose
        keys fit 16 bits; then every case's expected permutation equals it wherever the keys fit.
CENSUS  conditions on the cases, not measurements: the plan door changes form exactly once, the adversaries reach the heapsort
        fall-back in every way the device treats differently.
KD-TREE the core distances of the large-map checks come from a KD-tree; it equals the oracle's brute force."""
import os

import numpy as np
import pytest

import edge_order_cases as C
import tail_paths as tp
from oracle import hdbscan_ref as H, npsort_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _live(keys):
    return np.argsort(np.asarray(keys).astype(np.uint16))


def _numpy_has_a_scalar_u16_argsort():
    """np.argsort on uint16 keys reproduces every committed golden permutation whose keys fit 16 bits -> (ok, goldens compared)."""
    g = np.load(os.path.join(GOLDEN, 'npsort_golden.npz'))
    n_fit = 0
    for i in range(int(g['n'])):
        w, o = g['w_%d' % i], g['o_%d' % i]
        if w.min() >= 0 and C.fits_u16(w):
            n_fit += 1
            if not np.array_equal(_live(w), o):
                return False, n_fit
    return True, n_fit


def test_live_numpy_sorts_16_bit_keys_with_the_scalar_introsort():
    ok, n_fit = _numpy_has_a_scalar_u16_argsort()
    assert ok, ('numpy %s has no scalar 16-bit argsort: np.argsort(uint16 keys) does not reproduce the committed permutations of '
                'tests/golden/npsort_golden.npz, so it cannot serve as the second pin of oracle/npsort_ref.py' % np.__version__)
    assert n_fit >= 40                                        # (the goldens of 100 000 values do not fit; the adversaries do)


@pytest.mark.parametrize('family', C.FAMILIES)
def test_every_expected_permutation_is_live_numpys(family):
    """npsort_ref.argsort on every size of the family equals np.argsort of the same keys as uint16, wherever they fit ('topbit'
    does not: there the restatement is compared with a stable sort of the keys, which any correct order agrees with up to ties)."""
    assert _numpy_has_a_scalar_u16_argsort()[0], 'numpy %s has no scalar 16-bit argsort' % np.__version__
    cap = C.lds_cap()
    for n in C.sizes_of(family, cap):
        keys = C.family_keys(family, n)
        assert keys.dtype == np.uint32 and keys.shape == (n,)
        want = C.expected_order((family, n), keys)
        if family == 'topbit':
            assert n < 4 or int(keys.max()) >= 1 << 31, n
            assert np.array_equal(np.sort(want), np.arange(n)) and np.array_equal(keys[want], np.sort(keys)), n
        else:
            assert C.fits_u16(keys), (family, n)
            assert np.array_equal(want, _live(keys)), (family, n)


def test_every_adversarys_expected_permutation_is_live_numpys():
    assert _numpy_has_a_scalar_u16_argsort()[0], 'numpy %s has no scalar 16-bit argsort' % np.__version__
    adv = C.adversaries(C.lds_cap())
    assert tuple(adv) == C.ADVERSARY_LABELS
    for label, keys in adv.items():
        assert C.fits_u16(keys), label
        assert np.array_equal(C.expected_order(label, keys), _live(keys)), label


def test_killer_is_the_goldens_and_twin_leaves_both_halves_untouched():
    """killer(n) here is the definition tools/make_golden_hdbscan.py wrote the committed adversaries with (the three of 64, 300 and
    2 000 keys are the last goldens); the first partition of a twin puts the middle key in the middle and moves nothing else."""
    g = np.load(os.path.join(GOLDEN, 'npsort_golden.npz'))
    last = int(g['n']) - 3
    for j, n in enumerate((64, 300, 2000)):
        assert np.array_equal(C.killer(n), g['w_%d' % (last + j)].astype(np.float64)), n
    w = C.killer(300).astype(np.int64)
    t = C.twin(w)
    assert len(t) == 601 and t[300] == w.max() + 1 and np.array_equal(t[:300], w) and np.array_equal(t[301:] - t[300] - 1, w)
    order = np.asarray(npsort_ref.argsort(t.tolist()))
    assert order[300] == 300 and set(order[:300].tolist()) == set(range(300))


def test_the_plan_door_changes_form_exactly_once():
    from retargetvid_amd import ops
    forms = C.plan_forms()[1:]
    assert forms[0] and not forms[-1] and int((np.diff(forms.astype(np.int8)) != 0).sum()) == 1
    cap = C.lds_cap()
    assert 5000 <= cap <= 6500
    assert ops.sort_plan(cap)['in_lds'] == 1 and ops.sort_plan(cap + 1)['in_lds'] == 0
    for n in (1, 16, 17, cap, cap + 1, C.MAX_KEYS):
        assert ops.sort_plan(n)['depth'] == 2 * npsort_ref._msb(n), n
    sizes = {n for f in C.FAMILIES for n in C.sizes_of(f, cap)}
    assert set(range(1, 71)) <= sizes and {cap - 1, cap, cap + 1, cap + 2} <= sizes and set(C.LARGE_SIZES) <= sizes
    assert max(sizes) == C.MAX_KEYS and 255 * 255 - 1 in sizes


def test_the_adversaries_reach_the_heapsort_in_every_way_the_device_tells_apart():
    cap = C.lds_cap()
    ranges = {}
    for label, keys in C.adversaries(cap).items():
        st = {}
        C.expected_order(label, keys, st)
        assert st.get('heapsorts', 0) == len(st.get('ranges', ())) >= 1, label
        ranges[label] = st['ranges']
        for lo, n, cdepth in st['ranges']:
            assert cdepth < 0 and 0 <= lo and lo + n <= len(keys), label
    adv = C.adversaries(cap)
    assert max(len(r) for r in ranges.values()) >= 8                                        # an array with at least 8 heapsorts
    assert any(n <= 16 for r in ranges.values() for _, n, _ in r)                           # a heap-sorted range of at most 16 elements
    assert any(len({d for _, _, d in r}) < len(r) for r in ranges.values())                 # two ranges heap-sorted at the same cdepth
    assert any(len(adv[label]) == cap + 1 for label in ranges)                              # a heap-sorted range in an array of cap + 1 keys
    # ... and in both forms: the killers straddle the seam, the seam twin lies beyond it with many ranges
    assert len(adv['killer(cap)']) == cap and len(adv['killer(cap+1)']) == cap + 1
    assert len(adv['twin(killer(m)),2m+1>cap']) > cap and len(ranges['twin(killer(m)),2m+1>cap']) >= 8
    assert any(n <= 16 for _, n, _ in ranges['twin(killer(m)),2m+1>cap'])                   # a small heap-sorted range in global memory too


def test_the_maps_have_the_sizes_they_are_meant_to_have():
    cap = C.lds_cap()
    assert [int((m > 0).sum()) for m in C.seam_maps(cap)] == [cap + 1, cap + 2]
    counts = {name: int((C.large_map(name) > 0).sum()) for name in C.LARGE_MAP_NAMES}
    assert counts['255x255/all'] == 65025 and counts['187x250/all'] == 46750
    assert C.DENSE_RANGE[0] <= counts['140x250/holes'] <= C.DENSE_RANGE[1]
    assert min(counts.values()) > 9500 and sum(c > 30000 for c in counts.values()) == 6


@pytest.mark.parametrize('n_points', [200, 901, 2500])
def test_kdtree_core_distances_are_the_oracles(n_points):
    """scipy's KD-tree gives H.core_distances for the k of both published parameter sets (26 and 3) and for k = 1, on noise maps
    of 200 to 2 500 points (grids tie heavily at the k-th distance: the VALUE is the same whichever neighbour is taken)."""
    rng = np.random.RandomState(n_points)
    m = tp.noise_map_with_n_points(rng, 60, 90, n_points / 5400.0, n_points)
    X = np.argwhere(m > 0)
    ks = {H.effective_min_samples(len(X), CP['hdbscan_min'], CP['hdbscan_min_samples']) for CP in (tp.DEFAULT, tp.BEST_LIKE)} | {1}
    assert ks == {26, 3, 1}
    for k in sorted(ks):
        assert np.array_equal(C.kdtree_core(X, k), H.core_distances(X, k)), k


def test_the_edge_list_checker_accepts_the_oracles_prim_and_refuses_a_wrong_one():
    """mst_faults on H.prim_mst's own output: no fault; a weight off by one, a `to` repeated, a `from` that is not the last point:
    each is named.  (Prim's `from` is the point added last, not the one that achieves the minimum: on this map some weights are
    below the mutual reachability of the edge as written, which is why the checker takes the minimum over the visited points.)"""
    rng = np.random.RandomState(5)
    m = tp.noise_map_with_n_points(rng, 60, 90, 0.3, 1600)
    X = np.argwhere(m > 0)
    for k in (26, 3):
        core = H.core_distances(X, k)
        mst = np.stack(H.prim_mst(X, core), 1)
        assert C.mst_faults(X, core, mst) == []
        u, v, w = mst.T
        own = np.maximum(np.maximum(core[u], core[v]), ((X[u] - X[v]) ** 2).sum(1))
        assert (w <= own).all() and (w < own).any()
        for col, row, delta in ((2, 800, 1), (2, 801, -1), (1, 700, 0), (0, 600, 0)):
            bad = mst.copy()
            if delta:
                bad[row, col] += delta
            elif col == 1:
                bad[row, 1] = bad[row - 1, 1]
            else:
                bad[row, 0] = bad[row - 2, 1]
            assert C.mst_faults(X, core, bad), (k, col, row, delta)
        labels, ncl = C.back_half(mst, 5)
        assert C.same_partition(labels, H.hdbscan_labels(X, 5, k)) and ncl >= 1


def _introsort_with_another_depth_rule(keys, depth_add=0, push_right_on_equal=False, size_before_depth=False):
    """npsort_ref.argsort with one rule of the depth bookkeeping changed -- the three ways a device emulation can get it wrong
    without touching a bound: a depth limit of 2 msb + 1, the right side pushed when both sides are equally long, a popped range
    of at most 16 elements insertion-sorted although it is below the limit.  With all three off it is npsort_ref.argsort."""
    v = list(keys)
    num = len(v)
    a = list(range(num))
    if num < 2:
        return a
    pl, pr, stack = 0, num - 1, []
    cdepth = npsort_ref._msb(num) * 2 + depth_add
    while True:
        if cdepth < 0 and not (size_before_depth and pr - pl <= npsort_ref.SMALL_QUICKSORT):
            npsort_ref.aheapsort(v, a, pl, pr - pl + 1)
        else:
            while pr - pl > npsort_ref.SMALL_QUICKSORT:
                pm = pl + ((pr - pl) >> 1)
                if v[a[pm]] < v[a[pl]]:
                    a[pm], a[pl] = a[pl], a[pm]
                if v[a[pr]] < v[a[pm]]:
                    a[pr], a[pm] = a[pm], a[pr]
                if v[a[pm]] < v[a[pl]]:
                    a[pm], a[pl] = a[pl], a[pm]
                vp = v[a[pm]]
                pi, pj = pl, pr - 1
                a[pm], a[pj] = a[pj], a[pm]
                while True:
                    pi += 1
                    while v[a[pi]] < vp:
                        pi += 1
                    pj -= 1
                    while vp < v[a[pj]]:
                        pj -= 1
                    if pi >= pj:
                        break
                    a[pi], a[pj] = a[pj], a[pi]
                a[pi], a[pr - 1] = a[pr - 1], a[pi]
                cdepth -= 1
                if (pi - pl <= pr - pi) if push_right_on_equal else (pi - pl < pr - pi):
                    stack.append((pi + 1, pr, cdepth))
                    pr = pi - 1
                else:
                    stack.append((pl, pi - 1, cdepth))
                    pl = pi + 1
            for pi in range(pl + 1, pr + 1):
                vi = a[pi]
                vp = v[vi]
                pj = pi
                while pj > pl and vp < v[a[pj - 1]]:
                    a[pj] = a[pj - 1]
                    pj -= 1
                a[pj] = vi
        if not stack:
            break
        pl, pr, cdepth = stack.pop()
    return a


def test_each_wrong_depth_rule_changes_an_adversary_in_lds_and_one_in_global_memory():
    """The heap-sorted ranges of the plain killers and twins hold distinct keys: any correct sort orders them alike, and none of the
    three wrong depth rules changes their permutation.  The coarse killers have ties there: each rule changes the expected
    permutation of at least one of them at up to cap keys (the LDS form) and of one beyond (global memory), so the device test's
    comparison with npsort_ref fails for a device that has the rule wrong."""
    cap = C.lds_cap()
    adv = C.adversaries(cap)
    rules = {'depth limit 2 msb + 1': dict(depth_add=1), 'right side pushed on equal lengths': dict(push_right_on_equal=True),
             'size before depth': dict(size_before_depth=True)}
    changed = {name: set() for name in rules}
    for label, keys in adv.items():
        k = keys.astype(np.int64).tolist()
        want = C.expected_order(label, keys).tolist()
        assert _introsort_with_another_depth_rule(k) == want, label
        for name, kw in rules.items():
            if _introsort_with_another_depth_rule(k, **kw) != want:
                changed[name].add(label)
    for name, labels in changed.items():
        assert not any(label.startswith(('killer', 'twin(killer', 'twin(twin')) for label in labels), (name, labels)
        assert any(len(adv[label]) <= cap for label in labels), (name, 'no adversary in the LDS form', labels)
        assert any(len(adv[label]) > cap for label in labels), (name, 'no adversary in global memory', labels)
