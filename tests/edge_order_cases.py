"""Key arrays and maps for the edge sort (k_sort, Engine.argsort_u32: csrc/svc_tail.hip) and for what lies behind it, built on the
CPU for tests/test_edge_order_host.py and tests/test_gpu_edge_order.py (a helper module, not a conftest).

k_sort emulates numpy's unstable introsort so that equal MST weights reach the single-linkage pass in the reference's order
(oracle/npsort_ref.py).  The routine changes form with the number of keys -- insertion sort up to 16 elements, partition above,
working arrays in LDS up to a size that the plan door reports (ops.sort_plan; nothing here restates it), in global memory beyond,
heapsort for a range popped below the depth limit -- and its counters are 16 bits wide, with nothing to spare at 65 535 keys.
The cases below sit on every one of those seams:

  families   eight kinds of keys per size (FAMILIES); 'topbit' has keys with bit 31 set: the door takes any uint32 and compares unsigned
  sizes      every n from 1 to 70; cap - 1 .. cap + 2 around the last LDS size; seven sizes from 32 767 to 65 535 (LARGE_FAMILIES)
  adversaries  McIlroy's killer at cap and cap + 1 keys (one heap-sorted range, in LDS and in global memory) and twins of killers:
             twin(w) = w || [max + 1] || (w + max + 2).  The first partition of a twin takes the middle key as its pivot and leaves
             both halves as they were, so each half degenerates by itself one level further down: several heap-sorted ranges per
             array, in pairs of one depth, some of 16 elements or fewer.  The heap-sorted ranges of all of these hold DISTINCT
             keys, so coarse(w, g) adds ties there: up to 242 heap-sorted ranges per array whose result depends on which ranges
             the depth rule picks.
  maps       noise maps of cap + 1 and cap + 2 points (cap and cap + 1 edges: the seam in production), the six largest-geometry maps
             of tests/test_gpu_parity.py and one 140 x 250 blob with holes of 20 000 to 22 000 points.

Everything is seeded; an expected permutation is computed once per process (expected_order)."""
import functools

import numpy as np

from oracle import npsort_ref

FAMILIES = ('equal', 'two', 'five', 'forty', 'perm', 'asc', 'desc', 'topbit')
LARGE_FAMILIES = ('perm', 'asc', 'desc', 'equal', 'two', 'forty')
SMALL_SIZES = tuple(range(1, 71))
LARGE_SIZES = (32767, 32768, 32769, 50000, 65024, 65534, 65535)
SEAM_OFFSETS = (-1, 0, 1, 2)          # sizes cap + offset
MAX_KEYS = 65535                      # what the door accepts
SEAM_MAP_SHAPE = (80, 100)
DENSE_RANGE = (20000, 22000)


# ---- the plan door ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_forms():
    """bool [MAX_KEYS + 1]: in_lds of ops.sort_plan(n) for every n the door accepts (index 0 unused)."""
    import ctypes
    from retargetvid_amd import _lib, ops
    assert ops.SORT_PLAN_WORDS[0] == 'in_lds' and ops.sort_plan(1)['in_lds'] == 1
    door = _lib.load().svc_debug_sort_plan                   # (the entry ops.sort_plan wraps, called bare: 65 535 calls)
    words = (ctypes.c_int32 * len(ops.SORT_PLAN_WORDS))()
    ptr = ctypes.cast(words, ctypes.c_void_p)
    out = np.zeros(MAX_KEYS + 1, bool)
    for n in range(1, MAX_KEYS + 1):
        assert door(n, ptr, len(words)) == len(words), n
        out[n] = bool(words[0])
    return out


def lds_cap():
    """The last number of keys whose working arrays are in LDS, from the door."""
    forms = plan_forms()
    return int(np.nonzero(forms)[0][-1])


# ---- adversaries --------------------------------------------------------------------------------------------------------------
def killer(n):
    """McIlroy's adversary run against the restated introsort: a key array on which it degenerates, so that the
    depth limit is hit and popped ranges are heap-sorted.  -> float64 [n], whole numbers 0 .. n."""
    gas = n
    val = [gas] * n
    state = dict(nsolid=0, cand=0)

    class Item:
        __slots__ = ('i',)

        def __init__(self, i):
            self.i = i

        def __lt__(self, other):
            x, y = self.i, other.i
            if val[x] == gas and val[y] == gas:
                f = x if x == state['cand'] else y
                val[f] = state['nsolid']
                state['nsolid'] += 1
            if val[x] == gas:
                state['cand'] = x
            elif val[y] == gas:
                state['cand'] = y
            return val[x] < val[y]

    npsort_ref.argsort([Item(i) for i in range(n)])
    return np.array([v if v != gas else n for v in val], np.float64)


def twin(w):
    """w || [max + 1] || (w + max + 2): the median of three of the first partition sees low, pivot, high, the parked pivot comes
    back to the middle and both halves are left untouched, one level down."""
    w = np.asarray(w, np.int64)
    top = int(w.max())
    return np.concatenate([w, [top + 1], w + top + 2])


def coarse(w, g):
    """A killer with ties where the heapsort works: the keys the degenerate partitions resolve one by one (the 2 msb(n) + 2
    smallest) stay, the others are grouped g at a time.  A heap-sorted range of a plain killer holds distinct keys, which every
    correct sort orders alike; with ties the unstable heapsort and the partition + insertion sort leave different permutations, so
    WHICH ranges are heap-sorted -- the depth limit, the side that is pushed, depth before size -- shows in the result."""
    w = np.asarray(w, np.int64)
    r0 = 2 * npsort_ref._msb(len(w)) + 2
    return np.where(w >= r0, r0 + (w - r0) // g, w)


@functools.lru_cache(maxsize=None)
def _killer_u32(n):
    return killer(n).astype(np.uint32)


def adversaries(cap):
    """{label: uint32 keys}: the killers at cap and cap + 1 keys, the twins and the coarse killers (module docstring).  The twins
    at the seam have 2 m + 1 keys with m = (cap + 1) // 2: cap + 1 keys for an even cap, cap + 2 for an odd one -- in global
    memory either way."""
    m = (cap + 1) // 2
    out = {
        'killer(cap)': _killer_u32(cap),
        'killer(cap+1)': _killer_u32(cap + 1),
        'twin(killer(m)),2m+1>cap': twin(_killer_u32(m)),
        'twin(killer(300))': twin(_killer_u32(300)),
        'twin(twin(killer(1000)))': twin(twin(_killer_u32(1000))),
        'coarse(killer(1000),5)': coarse(_killer_u32(1000), 5),
        'coarse(killer(cap),5)': coarse(_killer_u32(cap), 5),
        'coarse(killer(cap),40)': coarse(_killer_u32(cap), 40),
        'coarse(killer(cap+1),4)': coarse(_killer_u32(cap + 1), 4),
        'twin(coarse(killer(m),5)),2m+1>cap': twin(coarse(_killer_u32(m), 5)),
    }
    return {k: np.ascontiguousarray(v, np.uint32) for k, v in out.items()}


ADVERSARY_LABELS = ('killer(cap)', 'killer(cap+1)', 'twin(killer(m)),2m+1>cap', 'twin(killer(300))', 'twin(twin(killer(1000)))',
                    'coarse(killer(1000),5)', 'coarse(killer(cap),5)', 'coarse(killer(cap),40)', 'coarse(killer(cap+1),4)',
                    'twin(coarse(killer(m),5)),2m+1>cap')


# ---- key families -------------------------------------------------------------------------------------------------------------
def family_keys(family, n):
    """uint32 [n] keys of one family, seeded by (family, n).  Every family but 'topbit' fits 16 bits at every n <= 65 535."""
    rng = np.random.RandomState(16 * n + FAMILIES.index(family))
    if family == 'equal':
        w = np.full(n, 7)
    elif family in ('two', 'five', 'forty'):
        w = rng.randint(1, {'two': 3, 'five': 6, 'forty': 41}[family], n)
    elif family == 'perm':
        w = rng.permutation(n)
    elif family in ('asc', 'desc'):
        w = np.sort(rng.randint(0, n // 2 + 2, n))           # runs of equal keys inside a sorted array
        if family == 'desc':
            w = w[::-1]
    else:                                                    # 'topbit': few values, half of them at 2^31 and above
        w = rng.randint(0, 5, n).astype(np.int64) + (rng.randint(0, 2, n).astype(np.int64) << 31)
    return np.ascontiguousarray(w, np.uint32)


def sizes_of(family, cap):
    """Every size a family is run at: 1 .. 70, the four seam sizes and, for LARGE_FAMILIES, the seven large ones."""
    out = list(SMALL_SIZES) + [cap + d for d in SEAM_OFFSETS]
    if family in LARGE_FAMILIES:
        out += list(LARGE_SIZES)
    return out


_EXPECTED = {}


def expected_order(label, keys, stats=None):
    """npsort_ref.argsort(keys) as int32, once per label and process (with a stats dict it is computed again, to fill it)."""
    if label not in _EXPECTED or stats is not None:
        _EXPECTED[label] = np.asarray(npsort_ref.argsort(np.asarray(keys, np.int64).tolist(), stats), np.int32)
    return _EXPECTED[label]


def fits_u16(keys):
    return len(keys) == 0 or int(np.max(keys)) <= 0xFFFF


# ---- maps ---------------------------------------------------------------------------------------------------------------------
def seam_maps(cap):
    """uint8 [2, 80, 100]: noise of cap + 1 and cap + 2 points -- cap and cap + 1 MST edges, k_sort's last LDS size and its first
    global one."""
    import tail_paths as tp
    h, w = SEAM_MAP_SHAPE
    assert cap + 2 < h * w
    rng = np.random.RandomState(cap)
    return np.stack([tp.noise_map_with_n_points(rng, h, w, (cap + 1) / float(h * w), n) for n in (cap + 1, cap + 2)])


LARGE_MAP_NAMES = tuple('%dx%d/%s' % (h, w, kind) for (h, w) in ((187, 250), (255, 255)) for kind in ('all', 'noise80', 'sine')) + ('140x250/holes',)


@functools.lru_cache(maxsize=None)
def _large_maps():
    out = {}
    rng = np.random.RandomState(91)                          # the maps of test_largest_geometries_up_to_65025_points...: same seed, same draws
    for (h, w) in ((187, 250), (255, 255)):
        ys, xs = np.mgrid[0:h, 0:w]
        out['%dx%d/all' % (h, w)] = np.full((h, w), 200, np.uint8)
        out['%dx%d/noise80' % (h, w)] = np.where(rng.rand(h, w) < 0.8, 220, 0).astype(np.uint8)
        out['%dx%d/sine' % (h, w)] = np.where(np.sin(xs / 4.0) * np.sin(ys / 3.0) > -0.7, 180, 0).astype(np.uint8)
    out['140x250/holes'] = dense_map_with_holes()
    return out


def large_map(name):
    return _large_maps()[name]


def dense_map_with_holes(seed=2200):
    """One 140 x 250 map in the style of test_gpu_parity._dense_maps' third kind: soft blobs thinned by noise, so that core
    distances vary from point to point; 20 000 to 22 000 points (the seed is advanced until the count lies there)."""
    ys, xs = np.mgrid[0:140, 0:250]
    rng = np.random.RandomState(seed)
    while True:
        m = np.zeros((140, 250), np.float32)
        for _ in range(rng.randint(2, 4)):
            cy, cx = rng.uniform(20, 120), rng.uniform(30, 220)
            ry, rx = rng.uniform(50, 90), rng.uniform(90, 160)
            m = np.maximum(m, 255 * np.exp(-(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2) * rng.uniform(0.6, 1.2)))
        m = m * (rng.rand(140, 250) < rng.uniform(0.6, 0.9))
        u = np.clip(m + rng.uniform(0, 30) * rng.rand(140, 250), 0, 255).astype(np.uint8)
        u[u < 120] = 0
        if DENSE_RANGE[0] <= int((u > 0).sum()) <= DENSE_RANGE[1]:
            return u


# ---- everything behind the MST, restated ------------------------------------------------------------------------------------------
def kdtree_core(X, k):
    """H.core_distances(X, k) by a KD-tree: the squared distance to the k-th other point, int64 [N]."""
    from scipy.spatial import cKDTree
    X = np.asarray(X, np.float64)
    d = cKDTree(X).query(X, k + 1)[0][:, k]
    return np.rint(d * d).astype(np.int64)


def mst_faults(X, core, mst):
    """An edge list [N - 1, 3] (from, to, weight) against what the library's Prim writes, without running it -> list of faults
    (empty: a spanning tree in Prim shape with exact weights):
      * the walk starts at point 0; every `from` is the point added last (so: already visited), every `to` is new;
      * every weight is the smallest mutual reachability max(core[t], core[v], d2(t, v)) between the new point v and the points t
        visited before it -- the value Prim holds for v when it takes it.  (Its `from` is the point added LAST, not the point that
        achieves the minimum, so max(core[u], core[v], d2(u, v)) of the edge as written only bounds the weight from above.)
        Any t that achieves or undercuts w lies within sqrt(w) of v: a KD-tree ball per point makes the minimum exact."""
    from scipy.spatial import cKDTree
    X = np.asarray(X, np.int64)
    core = np.asarray(core, np.int64)
    mst = np.asarray(mst, np.int64)
    n = len(X)
    bad = []
    if mst.shape != (n - 1, 3):
        return ['%s edges for %d points' % (mst.shape, n)]
    u, v, w = mst[:, 0], mst[:, 1], mst[:, 2]
    if u.min() < 0 or u.max() >= n or v.min() < 0 or v.max() >= n:
        return ['an end point outside 0 .. N - 1']
    pos = np.full(n, -1, np.int64)                           # the step at which a point is visited
    pos[0] = 0
    if len(np.unique(v)) != n - 1 or (v == 0).any():
        bad.append('the `to` column is not every point but 0 exactly once')
        return bad
    pos[v] = np.arange(1, n)
    if u[0] != 0 or not np.array_equal(u[1:], v[:-1]):
        bad.append('a `from` that is not the point added last')
    d2 = ((X[u] - X[v]) ** 2).sum(1)
    upper = np.maximum(np.maximum(core[u], core[v]), d2)
    if (w > upper).any():
        bad.append('%d weights above the mutual reachability of their own edge' % int((w > upper).sum()))
    tree = cKDTree(X.astype(np.float64))
    radius = np.sqrt(w.astype(np.float64)) * (1 + 1e-12) + 1e-9
    for s in range(0, n - 1, 4096):                          # balls in chunks: the pair lists stay small
        vs = v[s:s + 4096]
        balls = tree.query_ball_point(X[vs].astype(np.float64), radius[s:s + 4096])
        cnt = np.fromiter((len(b) for b in balls), np.int64, len(balls))
        t = np.fromiter((j for b in balls for j in b), np.int64, int(cnt.sum()))
        vv = np.repeat(vs, cnt)
        mr = np.maximum(np.maximum(core[t], core[vv]), ((X[t] - X[vv]) ** 2).sum(1))
        mr[pos[t] >= pos[vv]] = np.iinfo(np.int64).max       # not visited before v (v itself included)
        best = np.full(len(vs), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, np.repeat(np.arange(len(vs)), cnt), mr)
        wrong = best != w[s:s + 4096]
        if wrong.any():
            i = s + int(np.nonzero(wrong)[0][0])
            bad.append('%d weights of steps %d.. are not the minimum over the visited points (step %d: %d, minimum %d)'
                       % (int(wrong.sum()), s, i, int(w[i]), int(best[i - s])))
            break
    return bad


def back_half(mst, mcs, order=None):
    """The oracle's hierarchy on an edge list [N - 1, 3] (the device's own MST): H.single_linkage -> condense_tree ->
    select_and_label -> (labels [N], condensed clusters).  order: the numpy-order permutation of the weights when the caller has
    it already (else oracle/npsort_ref.py computes it)."""
    import tail_paths as tp
    from oracle import hdbscan_ref as H
    mst = np.asarray(mst, np.int64)
    left, right, weight, csize = H.single_linkage(mst[:, 0], mst[:, 1], mst[:, 2], order)
    rows = H.condense_tree(left, right, weight, csize, mcs)
    return H.select_and_label(rows, len(mst) + 1), tp.condensed_clusters(rows)


def same_partition(ref, got):
    """Labels equal up to renaming (noise is noise in both)."""
    ref, got = np.asarray(ref), np.asarray(got)
    if not np.array_equal(ref < 0, got < 0):
        return False
    pairs = {(a, b) for a, b in zip(ref[ref >= 0].tolist(), got[got >= 0].tolist())}
    return len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
