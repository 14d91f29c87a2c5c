"""NumPy predictor of the run-time paths of the tail (svc_cluster_center: csrc/svc_tail.hip), and the directed maps of
tests/test_tail_paths_host.py and tests/test_gpu_tail_paths.py (a helper module, not a conftest).

The tail chooses its code path per map, from the data.  With a map's point list, the crop parameters and the words of the plan
door (Engine.tail_plan -> svc_debug_tail_plan; tests/golden/tail_plan.json holds them for the shapes used here) the path is a
function of the map, and the frame header (ops.HDR_*) records which one was taken:

  k_core      k = min(N - 1, hdbscan_min_samples or hdbscan_min) (1 if 0).  A point with at least k other points within
              RING_R1 is answered by phase 1 (interior form: at least RING_R1 from every border; else the bounds-tested form),
              else with at least k within RING_R by phase 2, else by phase 3.  Phase 3 runs when one point needs it; its form
              follows from N: four register forms (one per CORE_REG_STEP points up to CORE_REG_MAX), the LDS loop up to
              core_lds_max, the global loop beyond.  Header: the last two k_core stamps are equal exactly when phase 3 did not run.
  hierarchy   k_tree_par's mode by N (TP_CAP, TP_CAP_BIG); it keeps the map when the condensed clusters fit its tables (cap_cl;
              cap_cl_huge beyond TP_CAP_BIG), else k_tree and k_finish redo it.  Header: HDR_TREE_PAR, HDR_NCLUSTERS,
              HDR_BACK_DONE.  k_tree (every map of the reference engine): the LDS form up to TREE_LDS_CAP points, retried in
              global memory beyond TREE_LDS_CLUSTERS clusters.

  k_sort      its form follows from the number of edges N - 1 alone and has a door of its own (ops.sort_plan ->
              svc_debug_sort_plan: working arrays in LDS or in the workspace, the depth limit): insertion sort up to 16 elements,
              partition above, heapsort for a range popped below the depth limit.  Its cases and their census live in
              tests/edge_order_cases.py, tests/test_edge_order_host.py and tests/test_gpu_edge_order.py; header: HDR_T_SORTED.

Nothing here restates a formula of plan_tail: every threshold is read from the plan dict.  What IS restated is the order of the
ring table (offsets sorted by squared distance, stable over dr then dc ascending), which decides the slot of a point's k-th hit;
its length is checked against the plan's n_ring / n_ring1."""
import functools
import json
import os

import numpy as np

from oracle import hdbscan_ref as H, pipeline_ref as P, tail_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLAN_FIXTURE = os.path.join(GOLDEN, 'tail_plan.json')

DEFAULT = P.init_crop_params()
# the k of k_core: 26 (default settings), 3 (best settings), 1, and N - 1 (hdbscan_min_samples at or above N)
K_SETS = {
    'k26': dict(DEFAULT),
    'k3': dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=3, select_sum=1),
    'k1': dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=1),
    'kN': dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=1000000),
}
K_OF = {'k26': 26, 'k3': 3, 'k1': 1, 'kN': 7}          # kN: maps of 8 points without a filler, k = N - 1 = 7
DIRECTED_SHAPE = (72, 100)
HOLE_SHAPE = (80, 80)
GLOBAL_SHAPE = (96, 96)
SEAM_SHAPE = (72, 72)
FULL_SHAPE = (140, 250)


# ---- the plan fixture -------------------------------------------------------------------------------------------------------
def plan_key(h, w, CP):
    return '%dx%d/%d' % (h, w, CP['hdbscan_min'])


def fixture_requests():
    """(h, w, CP) of every plan the host tests read from the fixture: the shapes of the directed cases and of the census, with
    every hdbscan_min they are used with (the plan depends on the shape, on hdbscan_min and on the handle's tail form)."""
    out = {}
    for shape in (DIRECTED_SHAPE, HOLE_SHAPE, GLOBAL_SHAPE, SEAM_SHAPE, FULL_SHAPE):
        for mcs in (2, 5, 26):
            out[plan_key(shape[0], shape[1], dict(hdbscan_min=mcs))] = (shape[0], shape[1], dict(DEFAULT, hdbscan_min=mcs))
    for name, CP, m in existing_maps():
        out.setdefault(plan_key(m.shape[0], m.shape[1], CP), (m.shape[0], m.shape[1], dict(DEFAULT, hdbscan_min=CP['hdbscan_min'])))
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(PLAN_FIXTURE) as f:
        return json.load(f)


def default_plan(h, w, CP):
    """The default engine's plan for maps of h x w with CP, from the fixture (the GPU test holds it equal to the door)."""
    assert CP.get('resize_factor', 1) == 1 and CP['clust_filt']
    return dict(_fixture()['plans'][plan_key(h, w, CP)])


# ---- k_core -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring_table(radius):
    """int [n, 3] (dr, dc, d2): the offsets within `radius`, sorted by d2, stable over dr then dc ascending."""
    offs = [(dr, dc, dr * dr + dc * dc) for dr in range(-radius, radius + 1) for dc in range(-radius, radius + 1)
            if 0 < dr * dr + dc * dc <= radius * radius]
    offs.sort(key=lambda o: o[2])          # (Python's sort is stable)
    return np.array(offs, np.int64)


def ring_of(plan):
    ring = ring_table(plan['RING_R'])
    assert len(ring) == plan['n_ring'] and int((ring[:, 2] <= plan['RING_R1'] ** 2).sum()) == plan['n_ring1']
    return ring


def disc_counts(occ, radius):
    """int [h, w]: other set cells within squared distance radius^2 of every cell (row runs of the disc over cumulative sums)."""
    occ = (np.asarray(occ) != 0).astype(np.int64)
    h, w = occ.shape
    R = int(radius)
    pad = np.zeros((h + 2 * R, w + 2 * R + 1), np.int64)
    pad[R:R + h, R + 1:R + 1 + w] = occ
    cs = np.cumsum(pad, axis=1)
    out = -occ
    for dr in range(-R, R + 1):
        half = int(np.floor(np.sqrt(R * R - dr * dr) + 1e-9))
        rows = cs[R + dr:R + dr + h]
        out = out + rows[:, R + half + 1:R + half + 1 + w] - rows[:, R - half:R - half + w]
    return out


def effective_k(n, CP):
    return H.effective_min_samples(n, CP['hdbscan_min'], CP['hdbscan_min_samples'])


def predict_core(clustered, CP, plan):
    """The k_core path of every point of a map (as the cluster filter sees it: thresholded, blended) -> dict:
    N, clustered (the map goes through the filter at all), k, phase int [N] (1 | 2 | 3, raster order), interior bool [N] (phase 1's
    form), counts {1: ., 2: ., 3: .}, phase3_runs, phase3_form ('regs8' | 'regs16' | 'regs24' | 'regs32' | 'lds' | 'global';
    None when phase 3 does not run)."""
    occ = np.asarray(clustered) != 0
    h, w = occ.shape
    assert (h, w) == (plan['h'], plan['w'])
    n = int(occ.sum())
    out = dict(N=n, clustered=bool(CP['clust_filt'] and n > CP['hdbscan_min'] + 1), k=None, phase=None, interior=None,
               counts={1: 0, 2: 0, 3: 0}, phase3_runs=False, phase3_form=None)
    if not out['clustered']:
        return out
    k = effective_k(n, CP)
    r1, r2 = plan['RING_R1'], plan['RING_R']
    c1, c2 = disc_counts(occ, r1)[occ], disc_counts(occ, r2)[occ]
    phase = np.where(c1 >= k, 1, np.where(c2 >= k, 2, 3))
    rr, cc = np.nonzero(occ)
    out.update(k=k, phase=phase, interior=(rr >= r1) & (rr < h - r1) & (cc >= r1) & (cc < w - r1),
               counts={p: int((phase == p).sum()) for p in (1, 2, 3)})
    out['phase3_runs'] = out['counts'][3] > 0
    if out['phase3_runs']:
        out['phase3_form'] = phase3_form(n, plan)
    return out


def phase3_form(n, plan):
    if n > plan['core_lds_max']:
        return 'global'
    if n > plan['CORE_REG_MAX']:
        return 'lds'
    return 'regs%d' % (8 * -(-n // plan['CORE_REG_STEP']))


def point_index(clustered, r, c):
    """Position of pixel (r, c) in the map's point list (raster order)."""
    occ = np.asarray(clustered) != 0
    assert occ[r, c]
    return int(occ.ravel()[:r * occ.shape[1] + c].sum())


def kth_ring_index(clustered, r, c, k, ring):
    """Index in the ring table of the k-th set neighbour of (r, c), -1 when fewer than k lie within the table."""
    occ = np.asarray(clustered) != 0
    h, w = occ.shape
    rr, cc = r + ring[:, 0], c + ring[:, 1]
    ok = (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
    hit = np.zeros(len(ring), bool)
    hit[ok] = occ[rr[ok], cc[ok]]
    idx = np.nonzero(hit)[0]
    return int(idx[k - 1]) if len(idx) >= k else -1


# ---- hierarchy --------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_hdbscan(clustered, CP):
    """oracle.hdbscan_ref on the map's points, once per (map, hdbscan_min, hdbscan_min_samples) -> dict(X, core, mst [N-1, 3],
    labels, rows (the condensed tree), nclusters)."""
    clustered = np.ascontiguousarray(clustered)
    key = (clustered.shape, clustered.tobytes(), CP['hdbscan_min'], CP['hdbscan_min_samples'])
    if key not in _ORACLE:
        X = np.argwhere(clustered > 0).astype(np.int64)
        labels, tree = H.hdbscan_labels(X, CP['hdbscan_min'], CP['hdbscan_min_samples'], return_tree=True)
        _ORACLE[key] = dict(X=X, core=tree['core'], mst=np.stack(tree['mst'], 1), labels=labels, rows=tree['rows'],
                            nclusters=condensed_clusters(tree['rows']))
    return _ORACLE[key]


def condensed_clusters(rows):
    """Clusters of the oracle's condensed tree: every id that is a parent of a row or a child of more than one point.  This is
    the count SVC_HDR_NCLUSTERS holds (tests/test_tail_paths_host.py pins it to tools/sim/tree_path.py's births + splits)."""
    return len({p for p, _, _, _ in rows} | {c for _, c, _, s in rows if s > 1})


def predict_hierarchy(n, nclusters, CP, plan, reference=False):
    """The hierarchy path of a clustered map of n points and nclusters condensed clusters -> dict(mode 0 | 1 | 2, cap, tree_par
    (HDR_TREE_PAR), back_done (HDR_BACK_DONE), tree_form (k_tree's, None when k_tree_par keeps the map: 'lds' | 'lds_retry' |
    'global')).  reference: the reference engine (k_tree takes every map, nothing is fused)."""
    mode = 0 if n <= plan['TP_CAP'] else (1 if n <= plan['TP_CAP_BIG'] else 2)
    cap = plan['cap_cl_huge'] if mode == 2 else plan['cap_cl']
    kept = not reference and nclusters <= cap
    form = None
    if not kept:
        form = 'global' if n > plan['TREE_LDS_CAP'] else ('lds' if nclusters <= plan['TREE_LDS_CLUSTERS'] else 'lds_retry')
    return dict(mode=mode, cap=cap, tree_par=int(kept), back_done=int(kept and not reference and bool(plan['fused'])), tree_form=form)


def header_agrees(hdr, core, hier=None, nclusters=None):
    """The words of a frame header (ops.HDR_* numbers) against a prediction -> list of disagreements (empty: the path was taken)."""
    from retargetvid_amd import ops
    bad = []
    if hdr[ops.HDR_N] != core['N']:
        bad.append('N %d, predicted %d' % (hdr[ops.HDR_N], core['N']))
    if bool(hdr[ops.HDR_CLUSTERED]) != core['clustered']:
        bad.append('CLUSTERED %d' % hdr[ops.HDR_CLUSTERED])
    if core['clustered']:
        s = hdr[ops.HDR_CORE_STAMP0:ops.HDR_CORE_STAMP0 + ops.HDR_CORE_STAMPS]
        if (s[1] != s[2]) != core['phase3_runs']:
            bad.append('k_core stamps %s, phase 3 predicted %s' % (list(s), core['phase3_runs']))
        if hier is not None:
            if hdr[ops.HDR_TREE_PAR] != hier['tree_par']:
                bad.append('TREE_PAR %d, predicted %d' % (hdr[ops.HDR_TREE_PAR], hier['tree_par']))
            if hdr[ops.HDR_BACK_DONE] != hier['back_done']:
                bad.append('BACK_DONE %d, predicted %d' % (hdr[ops.HDR_BACK_DONE], hier['back_done']))
        if nclusters is not None and hdr[ops.HDR_NCLUSTERS] != nclusters:
            bad.append('NCLUSTERS %d, predicted %d' % (hdr[ops.HDR_NCLUSTERS], nclusters))
    return bad


# ---- directed k_core maps ---------------------------------------------------------------------------------------------------
POSITIONS = ('interior', 'top', 'bottom', 'left', 'right', 'tl', 'tr', 'bl', 'br')
PHASE1_KINDS = ('d16', 'slot7', 'slot0')          # the k-th hit at d2 = RING_R1^2; on the last slot of a group of eight; on the first of the next
PHASE2_KINDS = ('d17', 'd400_20_0', 'd400_12_16', 'd400_16_12', 'lane63', 'lane0', 'step255', 'step256')
ANSWERS = ('lo', 'twice_lo', 'above_twice_lo')    # phase 3's answer at RING_R^2 + 1, at twice that, at the next distance a grid has


def _position(shape, pos):
    h, w = shape
    return {'interior': (h // 2, 30), 'top': (2, 30), 'bottom': (h - 3, 30), 'left': (h // 2, 3), 'right': (h // 2, w - 4),
            'tl': (0, 0), 'tr': (0, w - 1), 'bl': (h - 1, 0), 'br': (h - 1, w - 1)}[pos]


def _in_bounds(shape, r, c, ring):
    rr, cc = r + ring[:, 0], c + ring[:, 1]
    return (rr >= 0) & (rr < shape[0]) & (cc >= 0) & (cc < shape[1])


def _filler(m, r, c):
    """36 points far from (r, c) and from everything within 22 px of it, so that the map is clustered whatever hdbscan_min."""
    h, w = m.shape
    c0 = w - 20 if c < w // 2 else 10
    r0 = h // 2 - 3
    assert (c0 - c) ** 2 > 45 ** 2 or (c0 + 5 - c) ** 2 > 45 ** 2
    m[r0:r0 + 6, c0:c0 + 6] = 180


def _decoys(m, r, c, reach):
    """Beside a left or right border: points where an offset that leaves the map sideways would land if its column were not
    tested (the far end of the rows within the ring table's reach).  They are most of a map's width away from (r, c): no
    neighbour count of the target moves."""
    h, w = m.shape
    rows = slice(max(r - reach - 1, 0), min(r + reach + 2, h))
    if c < reach:
        m[rows, w - reach:] = 150
    if c >= w - reach:
        m[rows, :reach] = 150


def target_map(shape, pos, k, kth_index, ring, filler=True):
    """A map whose point at `pos` has its k-th neighbour at ring[kth_index] exactly: k - 1 hits spread evenly over the in-bounds
    offsets below it, every other offset up to it empty -> (map, (r, c)), or None when the position has not enough offsets."""
    r, c = _position(shape, pos)
    inb = _in_bounds(shape, r, c, ring)
    if kth_index < 0 or not inb[kth_index]:
        return None
    below = np.nonzero(inb[:kth_index])[0]
    if len(below) < k - 1:
        return None
    pick = below[(np.arange(k - 1) * len(below)) // max(k - 1, 1)] if k > 1 else below[:0]
    m = np.zeros(shape, np.uint8)
    m[r, c] = 255
    for i in list(pick) + [kth_index]:
        m[r + ring[i, 0], c + ring[i, 1]] = 200
    if filler:
        _filler(m, r, c)
        _decoys(m, r, c, int(ring[:, 0].max()))
    return m, (r, c)


def _first_index(shape, pos, k, ring, pred, lo=0, hi=None):
    r, c = _position(shape, pos)
    inb = _in_bounds(shape, r, c, ring)
    for i in range(lo, len(ring) if hi is None else hi):
        if inb[i] and pred(i) and int(inb[:i].sum()) >= k - 1:
            return i
    return -1


def _offset_index(ring, dr, dc):
    return int(np.nonzero((ring[:, 0] == dr) & (ring[:, 1] == dc))[0][0])


def phase1_cases(kname, plan):
    """[(label, map, (r, c), kth ring index)] of the directed phase-1 maps for one k: PHASE1_KINDS x POSITIONS, less what a
    position cannot hold (a corner has 16 offsets within RING_R1: no k = 26 there)."""
    ring, k, n1 = ring_of(plan), K_OF[kname], plan['n_ring1']
    shape = (plan['h'], plan['w'])
    r1sq = plan['RING_R1'] ** 2
    out = []
    for pos in POSITIONS:
        for kind in PHASE1_KINDS:
            pred = {'d16': lambda i: ring[i, 2] == r1sq, 'slot7': lambda i: i % 8 == 7, 'slot0': lambda i: i % 8 == 0 and i >= 8}[kind]
            got = target_map(shape, pos, k, _first_index(shape, pos, k, ring, pred, hi=n1), ring, filler=kname != 'kN')
            if got is not None:
                out.append(('%s/%s/%s' % (kname, kind, pos), got[0], got[1], kth_ring_index(got[0], got[1][0], got[1][1], k, ring)))
    return out


def phase2_cases(kname, plan):
    """[(label, map, (r, c), kth ring index)] of the directed phase-2 maps for one k: PHASE2_KINDS at an interior point, and a
    point in every corner (three quarters of the ring out of bounds) with its k-th hit on the last offset it has."""
    ring, k, n1 = ring_of(plan), K_OF[kname], plan['n_ring1']
    shape = (plan['h'], plan['w'])
    r2sq = plan['RING_R'] ** 2
    out = []
    for kind in PHASE2_KINDS:
        if kind == 'd17':
            idx = n1                                                     # the first offset beyond phase 1's
        elif kind.startswith('d400'):
            dr, dc = (int(v) for v in kind.split('_')[1:])
            assert dr * dr + dc * dc == r2sq
            idx = _offset_index(ring, dr, dc)
        else:
            want = {'lane63': 63, 'lane0': 64, 'step255': 255, 'step256': 256}[kind]
            idx = want if want >= n1 else -1
        got = target_map(shape, 'interior', k, idx, ring, filler=kname != 'kN')
        if got is not None:
            out.append(('%s/%s/interior' % (kname, kind), got[0], got[1], idx))
    for pos in ('tl', 'tr', 'bl', 'br'):
        r, c = _position(shape, pos)
        idx = int(np.nonzero(_in_bounds(shape, r, c, ring))[0][-1])
        got = target_map(shape, pos, k, idx, ring, filler=kname != 'kN')
        if got is not None:
            out.append(('%s/corner/%s' % (kname, pos), got[0], got[1], idx))
    return out


def next_grid_distance(d2):
    """The smallest sum of two squares above d2 -> (d2', (dr, dc))."""
    t = d2 + 1
    while True:
        for a in range(int(np.sqrt(t)) + 1):
            b = int(round(np.sqrt(t - a * a)))
            if a * a + b * b == t and a <= b:
                return t, (a, b)
        t += 1


def answer_cases(kname, plan):
    """[(label, map, (r, c), expected core distance)] phase 3's answer positions for one k: the target's k-th neighbour at exactly
    RING_R^2 + 1 (the gallop's lower bound), at twice that (its first probe) and at the next distance above (the first probe fails)."""
    ring, k = ring_of(plan), K_OF[kname]
    shape = (plan['h'], plan['w'])
    lo = plan['RING_R'] ** 2 + 1
    out = []
    for name in ANSWERS:
        d2 = {'lo': lo, 'twice_lo': 2 * lo}.get(name)
        if d2 is None:
            d2, (dr, dc) = next_grid_distance(2 * lo)
        else:
            e, (dr, dc) = next_grid_distance(d2 - 1)
            assert e == d2, 'no grid offset at squared distance %d' % d2
        r, c = _position(shape, 'interior')
        inb = np.nonzero(_in_bounds(shape, r, c, ring))[0]
        pick = inb[(np.arange(k - 1) * len(inb)) // max(k - 1, 1)] if k > 1 else inb[:0]
        m = np.zeros(shape, np.uint8)
        m[r, c] = 255
        for i in pick:
            m[r + ring[i, 0], c + ring[i, 1]] = 200
        m[r + dr, c + dc] = 190
        if kname != 'kN':
            _filler(m, r, c)
            assert (shape[1] - 20 - c) ** 2 > d2
        out.append(('%s/answer_%s' % (kname, name), m, (r, c), d2))
    return out


DIAGONAL_CP = dict(DEFAULT, hdbscan_min=2, hdbscan_min_samples=4)


def diagonal_case(shape):
    """Four points, two of them in opposite corners, k = N - 1 = 3: a corner's answer is the map's diagonal, phase 3's upper bound."""
    h, w = shape
    m = np.zeros(shape, np.uint8)
    m[0, 0] = m[0, 1] = m[h - 1, w - 2] = 200
    m[h - 1, w - 1] = 255
    return m, (h - 1) ** 2 + (w - 1) ** 2


def hole_map(shape, n, seed, radius=21):
    """n points: one in the middle of a hole of `radius` px, n - 1 scattered over the rest of the map -> (map, (r, c))."""
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w]
    r, c = h // 2, w // 2
    free = np.flatnonzero(((ys - r) ** 2 + (xs - c) ** 2 > radius * radius).ravel())
    assert len(free) >= n - 1
    rng = np.random.RandomState(seed)
    m = np.zeros(h * w, np.uint8)
    sel = rng.permutation(len(free))[:n - 1]
    m[free[sel]] = rng.randint(121, 250, n - 1)
    m = m.reshape(h, w)
    m[r, c] = 255
    return m, (r, c)


def hole_cases(kname, plan):
    """[(label, map, (r, c), phase 3 form)]: maps of N points at and one above every register form's last size, one point of each
    alone in a hole wider than the ring table."""
    out = []
    for n in register_form_counts(plan):
        m, at = hole_map((plan['h'], plan['w']), n, 7 * n)
        out.append(('%s/hole/N%d' % (kname, n), m, at, phase3_form(n, plan)))
    return out


def loop_maps(plan):
    """(maps [2], (r, c)): hole maps of core_lds_max and core_lds_max + 1 points -- phase 3's LDS loop and its global loop."""
    got = [hole_map((plan['h'], plan['w']), n, 11 * n) for n in (plan['core_lds_max'], plan['core_lds_max'] + 1)]
    return np.stack([g[0] for g in got]), got[0][1]


def register_form_counts(plan):
    """N at and one above every register form's last size."""
    step = plan['CORE_REG_STEP']
    return [n for i in range(1, plan['CORE_REG_MAX'] // step + 1) for n in (i * step, i * step + 1)]


# ---- directed hierarchy maps ------------------------------------------------------------------------------------------------
def tile_map(shape, n_tiles, th, tw, seed, gap=1):
    """n_tiles tiles of th x tw set pixels on a grid with `gap` empty cells between neighbours, at seeded random grid positions;
    tile 0 holds 255, the others distinct-ish values from 121 up.  With hdbscan_min <= th * tw < 2 * hdbscan_min and
    hdbscan_min_samples = 1 every tile is one leaf of the condensed tree and every union of tiles a true split: 2 * n_tiles - 1
    condensed clusters."""
    h, w = shape
    rows, cols = (h + gap) // (th + gap), (w + gap) // (tw + gap)
    assert rows * cols >= n_tiles, (shape, n_tiles)
    cells = np.random.RandomState(seed).permutation(rows * cols)[:n_tiles]
    m = np.zeros(shape, np.uint8)
    for i, cell in enumerate(cells):
        r0, c0 = (cell // cols) * (th + gap), (cell % cols) * (tw + gap)
        m[r0:r0 + th, c0:c0 + tw] = 255 if i == 0 else 121 + (i * 37) % 130
    return m


def tiles_at_cap(cap):
    """The largest tile count whose 2 T - 1 clusters fit `cap`, and the next."""
    t = (cap + 1) // 2
    return t, t + 1


# (mode of k_tree_par, crop parameters, tile height, width): N <= TP_CAP, <= TP_CAP_BIG, beyond
TABLE_SEAMS = {
    0: (dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=1), 2, 3),
    1: (dict(DEFAULT, hdbscan_min=26, hdbscan_min_samples=1), 5, 6),
    2: (dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=1), 2, 3),
}


def table_seam_maps(mode, plan):
    """(CP, [map at the cap, map above it], [tile counts]) for one mode of k_tree_par on the plan's shape."""
    CP, th, tw = TABLE_SEAMS[mode]
    cap = plan['cap_cl_huge'] if mode == 2 else plan['cap_cl']
    counts = tiles_at_cap(cap)
    return CP, [tile_map((plan['h'], plan['w']), t, th, tw, 100 * mode + j) for j, t in enumerate(counts)], list(counts)


def tree_cluster_seam_maps(plan):
    """(CP, maps, tile counts): condensed clusters on both sides of k_tree's LDS tables, at N <= TREE_LDS_CAP."""
    CP, th, tw = TABLE_SEAMS[0]
    counts = tiles_at_cap(plan['TREE_LDS_CLUSTERS'])
    return CP, [tile_map((plan['h'], plan['w']), t, th, tw, 300 + j) for j, t in enumerate(counts)], list(counts)


MIXED_FLAGS = np.array([1, 1, 1, 0], np.uint8)


def mixed_call_maps(plan):
    """(CP, raw maps [4], flags): maps at and above k_tree_par's tables alternate in one blend chain.  All four share one tile
    grid and their first tiles (the same seed), so the kept tile of a map (tile 0: the highest value) lies on a tile of the next
    and the blend leaves the next map's tile count alone."""
    CP, th, tw = TABLE_SEAMS[0]
    at, over = tiles_at_cap(plan['cap_cl'])
    maps = np.stack([tile_map((plan['h'], plan['w']), t, th, tw, 400) for t in (at, over, at, over)])
    return CP, maps, MIXED_FLAGS


def blended_inputs(maps, flags, CP):
    """What the cluster filter sees of every map of a call (thresholded, blended from its final predecessor), by the oracle ->
    (clustered [n, h, w], final maps, dx, dy)."""
    ref = maps.copy()
    T.threshold(ref, CP['t_threshold'])
    seen = np.empty_like(ref)
    for i in range(len(ref)):
        seen[i] = ref[i]
        ref[i] = T.clustering_filt(ref[i], CP, labels_fn=lambda X, mcs, ms, m=seen[i].copy(): oracle_hdbscan(m, CP)['labels'])
        if i + 1 < len(ref) and flags is not None and flags[i]:
            ref[i + 1] = T.blend_next(ref[i], ref[i + 1])
    dx, dy = T.centers(np.ascontiguousarray(np.transpose(ref, (1, 2, 0))), CP)
    return seen, ref, dx, dy


def noise_map_with_n_points(rng, h, w, dens, n):
    """Noise with random pixels cleared or set until exactly n are set (value 200)."""
    m = rng.rand(h, w) < dens
    while int(m.sum()) != n:
        want = int(m.sum()) < n
        ys, xs = np.nonzero(m != want)
        j = rng.randint(len(ys))
        m[ys[j], xs[j]] = want
    return (m * 200).astype(np.uint8)


def point_seam_maps(plan):
    """Three maps of TP_CAP - 1, TP_CAP and TP_CAP + 1 points on the plan's shape (SEAM_SHAPE: noise dense enough for the condensed
    clusters to stay below the tables under both parameter sets)."""
    h, w = plan['h'], plan['w']
    rng = np.random.RandomState(plan['TP_CAP'])
    return np.stack([noise_map_with_n_points(rng, h, w, plan['TP_CAP'] / float(h * w), n)
                     for n in (plan['TP_CAP'] - 1, plan['TP_CAP'], plan['TP_CAP'] + 1)])


BEST_LIKE = dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=3, select_sum=1)


# ---- the maps the existing tail tests generate (census) ---------------------------------------------------------------------
def existing_maps():
    """(test, CP, thresholded map) for the maps of the tail tests of tests/test_gpu_parity.py, as their generators give them
    (same seeds, same arguments).  Cut blends are left out: a blended map is the union of two of these."""
    import test_gpu_parity as G
    out = []

    def add(test, CPs, maps):
        for CP in CPs:
            for m in maps:
                out.append((test, CP, T.threshold(np.array(m, np.uint8, copy=True), CP['t_threshold'])))

    g = np.load(os.path.join(GOLDEN, 'unisal_golden.npz'))
    base = np.transpose(g['smaps_u8'], (2, 0, 1)).copy()
    rng = np.random.RandomState(3)
    extra = [np.zeros((140, 250), np.uint8)]
    m = np.zeros((140, 250), np.uint8); m[10:13, 10:14] = 200; extra.append(m)
    m = np.zeros((140, 250), np.uint8); m[3:6, 3:12] = 200; extra.append(m)
    m = np.zeros((140, 250), np.uint8); m[3:6, 3:12] = 200; m[8, 3] = 130; extra.append(m)
    m = (rng.rand(140, 250) < 0.03) * rng.randint(120, 256, (140, 250)); m[50:80, 100:160] = 250
    extra.append(m.astype(np.uint8))
    m = base[1].copy(); m[m < 60] = 0; extra.append(m)
    extra.append(np.full((140, 250), 200, np.uint8))
    add('tail_bit_exact_default_settings', [DEFAULT], list(base) + extra)
    big, small = G._adversarial_maps()
    add('prim_rounds_and_parallel_hierarchy', [DEFAULT, dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=3)], big)
    add('prim_rounds_and_parallel_hierarchy', [dict(DEFAULT, hdbscan_min=5, hdbscan_min_samples=3), dict(DEFAULT, hdbscan_min=2, hdbscan_min_samples=1)], small)
    rng = np.random.RandomState(5)
    maps = []
    for s in range(6):
        m = np.zeros((140, 250), np.uint8)
        for _ in range(rng.randint(1, 5)):
            cy, cx, ry, rx = rng.randint(15, 125), rng.randint(20, 230), rng.randint(4, 14), rng.randint(4, 20)
            ys, xs = np.mgrid[0:140, 0:250]
            m[(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2) < 1] = rng.randint(90, 256)
        m[rng.rand(140, 250) < 0.004] = rng.randint(90, 256)
        maps.append(m)
    add('tail_bit_exact_other_parameters', [dict(DEFAULT, t_threshold=90, hdbscan_min=5, hdbscan_min_samples=3, select_sum=1), DEFAULT,
                                            dict(DEFAULT, hdbscan_min=40, hdbscan_min_samples=10)], maps)
    rng = np.random.RandomState(8)
    for (h, w) in [(187, 250), (250, 140), (33, 47)]:
        m = np.zeros((3, h, w), np.uint8)
        m[0, h // 4:h // 2, w // 4:w // 2] = 200
        m[1][rng.rand(h, w) < 0.02] = 180
        m[2, :, :] = (rng.rand(h, w) < 0.5) * 150
        add('tail_ragged_sizes_and_sparse_points', [DEFAULT], m)
    rng = np.random.RandomState(2024)
    for trial, (mcs, ms, ssum, close) in enumerate([(26, None, 2, True), (5, 3, 1, True), (12, 4, 2, False), (3, 2, 1, True)]):
        h, w = int(rng.randint(24, 70)), int(rng.randint(24, 90))
        maps = np.zeros((8, h, w), np.uint8)
        ys, xs = np.mgrid[0:h, 0:w]
        for i in range(8):
            m = rng.rand(h, w) < rng.choice([0.0, 0.03, 0.15, 0.5])
            for _ in range(rng.randint(0, 4)):
                cy, cx, ry, rx = rng.randint(0, h), rng.randint(0, w), rng.randint(2, 12), rng.randint(2, 16)
                m |= (((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2) < 1
            if i == 5:
                m = (xs % 4 == 0)
            maps[i] = np.where(m, rng.randint(121, 256, (h, w)), rng.randint(0, 120, (h, w))).astype(np.uint8)
        rng.rand(8)                                                       # (the test draws its flags here)
        add('tail_randomised_maps_bit_exact', [dict(DEFAULT, hdbscan_min=mcs, hdbscan_min_samples=ms)], maps)
    m = np.full((1, 140, 250), 200, np.uint8)
    m[0, 40:60, 100:130] = 0
    m[0, 0, 0:10] = 0
    add('tail_maximum_size_all_pixels_set', [DEFAULT], m)
    both = [DEFAULT, BEST_LIKE]
    add('maps_beyond_8192_points', both, G._dense_maps(np.random.RandomState(77), 24, 8500, 22000))
    add('maps_beyond_8192_points', [DEFAULT], G._dense_maps(np.random.RandomState(78), 1, 8300, 9500))
    rng = np.random.RandomState(8192)
    add('seam_at_8192_points', both, [G._noise_map_with_n_points(rng, 96, 96, 0.9, n) for n in (8191, 8192, 8193, 8256)])
    rng = np.random.RandomState(91)
    for (h, w) in ((187, 250), (255, 255)):
        maps = np.zeros((3, h, w), np.uint8)
        maps[0] = 200
        maps[1] = np.where(rng.rand(h, w) < 0.8, 220, 0)
        ys, xs = np.mgrid[0:h, 0:w]
        maps[2] = np.where(np.sin(xs / 4.0) * np.sin(ys / 3.0) > -0.7, 180, 0)
        add('largest_geometries_up_to_65025_points', [DEFAULT], maps)
    rng = np.random.RandomState(31)
    for (h, w, n) in ((140, 250, 48), (35, 62, 60), (187, 250, 24), (255, 255, 12)):
        maps = G._fuzz_maps(rng, n, h, w)
        rng.rand(n)                                                       # (the test draws its flags here)
        add('new_tail_kernels_equal_the_round2_kernels', both, maps)
    return out


CENSUS_ORACLE_N = 5000          # cluster counts are taken up to here (the oracle is O(N^2))
CENSUS_PATHS = ('k_core phase 1, interior form', 'k_core phase 1, border form', 'k_core phase 2', 'k_core phase 3: regs8',
                'k_core phase 3: regs16', 'k_core phase 3: regs24', 'k_core phase 3: regs32', 'k_core phase 3: lds',
                'k_core phase 3: global', 'k_core: every point in phase 3', 'k_tree_par mode 0 (N <= TP_CAP)',
                'k_tree_par mode 1 (N <= TP_CAP_BIG)', 'k_tree_par mode 2 (beyond)', 'N within 1 of TP_CAP', 'N within 1 of TP_CAP_BIG',
                'mode 0: kept', 'mode 0: handed to k_tree', 'mode 1: kept', 'mode 1: handed to k_tree',
                'clusters within 2 of the cap', 'k_tree LDS form retried (clusters > TREE_LDS_CLUSTERS)')


def census(entries):
    """Maps per path over (test, CP, thresholded map) entries -> (counts {path: maps}, clustered maps, maps with a cluster count)."""
    counts = dict.fromkeys(CENSUS_PATHS, 0)
    n_clustered = n_counted = 0
    for test, CP, m in entries:
        plan = default_plan(m.shape[0], m.shape[1], CP)
        core = predict_core(m, CP, plan)
        if not core['clustered']:
            continue
        n_clustered += 1
        n = core['N']
        one = core['phase'] == 1
        counts['k_core phase 1, interior form'] += bool((one & core['interior']).any())
        counts['k_core phase 1, border form'] += bool((one & ~core['interior']).any())
        counts['k_core phase 2'] += core['counts'][2] > 0
        if core['phase3_runs']:
            counts['k_core phase 3: ' + core['phase3_form']] += 1
        counts['k_core: every point in phase 3'] += core['counts'][3] == n
        mode = predict_hierarchy(n, 0, CP, plan)['mode']
        counts[('k_tree_par mode 0 (N <= TP_CAP)', 'k_tree_par mode 1 (N <= TP_CAP_BIG)', 'k_tree_par mode 2 (beyond)')[mode]] += 1
        counts['N within 1 of TP_CAP'] += abs(n - plan['TP_CAP']) <= 1
        counts['N within 1 of TP_CAP_BIG'] += abs(n - plan['TP_CAP_BIG']) <= 1
        if n <= CENSUS_ORACLE_N:
            n_counted += 1
            nc = oracle_hdbscan(m, CP)['nclusters']
            hier = predict_hierarchy(n, nc, CP, plan)
            counts['mode %d: %s' % (mode, 'kept' if hier['tree_par'] else 'handed to k_tree')] += 1
            counts['clusters within 2 of the cap'] += abs(nc - hier['cap']) <= 2
            counts['k_tree LDS form retried (clusters > TREE_LDS_CLUSTERS)'] += (not hier['tree_par'] and hier['tree_form'] == 'lds_retry')
    return counts, n_clustered, n_counted
