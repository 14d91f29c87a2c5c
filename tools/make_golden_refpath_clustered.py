"""tests/golden/refpath_clustered_golden.npz: the reference's OWN code around its cluster filter, run in the BUILD CONTAINER ONLY.

Part A  whole runs of the reference's smart_vid_crop (smartVidCrop.py:2218-2614) through its pickle door with clust_filt = True,
        op_close = False and resize_factor = 1.0, under the stubs of tools/make_golden_refpath.py (imported, not copied).  With
        these settings sc_clustering_filt (:1062-1161) calls no cv2 function but getTickCount, and its only use of the clusterer
        is fit_predict(X).  What runs is the reference's glue -- the np.sum == 0 return, the N > hdbscan_min + 1 gate, n_clusters
        without noise, max / sum weights, weights.index(max(weights)), the zeroing of every other point -- and the clustering loop
        of smart_vid_crop (:2359-2373) with its cut-adjacent blend, then centres, fill, focus stability, series and windows ON
        THE FILTERED MAPS.
Part B  direct calls of the reference's sc_clustering_filt with hand-made label vectors (ties, equal sums, losing label 0, all
        noise, the point-count gates, a sum past 2**16).

THE LABELS ARE NOT THE REFERENCE'S.  hdbscan 0.8.26 is not on this machine.  The stand-in for hdbscan.HDBSCAN is a class that
records its constructor keywords; its fit_predict(X) records X and returns the labels of scikit-learn's HDBSCAN for X, driven as
tools/fuzz_hdbscan_vs_sklearn.py::sk_labels drives it (min_samples + 1, metric sqeuclidean, brute), in a process with numpy's
SIMD argsort disabled: a child of this one (`--labels`, started with that file's NPY_DISABLE_CPU_FEATURES), so that the
reference itself runs on numpy as it is -- its LOESS differs by 1e-10 px where numpy's SIMD loops are off.  scikit-learn's port
is the project's declared proxy for the library (oracle/hdbscan_ref.py); the labels in the fixture are data from that proxy, and
in part B they are made by hand.  The generator also runs oracle.hdbscan_ref.hdbscan_labels on every X and refuses to write a
fixture where the two differ.

It enforces the caps of the census (CAPS below; counted by tests/refpath_clustered_cases.py::census, the one copy the tests
assert again) and refuses otherwise, and prints every seed it passed over (none for the committed fixture).  The fixture holds arrays and strings of settings only;
tests/refpath_clustered_cases.py reads it back.  Nothing at test, bench or smoke time imports this file, except the staleness test
of tests/test_refpath_clustered_host.py, which runs where the reference tree is present.

Run from the repo root:  python tools/make_golden_refpath_clustered.py <directory of the reference's smartVidCrop.py>"""
import json
import os
import subprocess
import sys

# (tools/fuzz_hdbscan_vs_sklearn.py::DISABLE: that file re-launches itself on import unless the environment already holds this)
DISABLE = 'AVX512F AVX512CD AVX512VL AVX512BW AVX512DQ AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR AVX2 FMA3'

import numpy as np                                   # noqa: E402

_TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _TOOLS)
sys.path.insert(0, os.path.dirname(_TOOLS))
import make_golden_refpath as G                      # noqa: E402
from make_golden_refpath import load_reference      # noqa: E402,F401
sys.path.insert(0, os.path.join(os.path.dirname(_TOOLS), 'tests'))
import refpath_clustered_cases as RCC                # noqa: E402  (the census is the reader's: one copy for generator and tests)
from oracle import hdbscan_ref as H, pipeline_ref as P              # noqa: E402

FIX = dict(op_close=False, resize_factor=1.0)
SETS = {'default_km': (False, dict(FIX)),
        'default_argmax': (False, dict(FIX, com_km=False)),
        'default_sum': (False, dict(FIX, select_sum=1)),
        'best_argmax': (True, dict(FIX, com_km=False)),
        'best_km': (True, dict(FIX, com_km=True))}
SIZES = [(640, 360), (360, 640)]
SQUARE = {7: 52, 15: 46, 22: 64}                     # case -> frames: the three short 720 x 720 videos (250 x 250 maps)
N_CASES = 24
MAX_POINTS = 3000
# (family, wanted scene starts as selected indices; negative: from fc_sel)
FAMILIES = [('no_cut', []), ('cut_at_sel_1', [1]), ('cut_at_fc_sel_2', [-2]), ('cut_at_fc_sel_3', [-3]), ('cuts_one_apart', [5, 6]),
            ('cuts_two_apart', [4, 6]), ('empty_chain_start', [5]), ('empty_chain_middle', [6]), ('empty_chain_end', [4]),
            ('wrap', [7]), ('gates', [8]), ('two_cuts', [3, 9])]
CAPS = dict(tied=12, tied3=4, not_raster_first=4, not_largest=4, sum_not_label0=6, chains3=8, chains5=2, blends_after_loss=6,
            wraps=2, lt_videos=2)


# ---- the labels -----------------------------------------------------------------------------------------------------------------
def labels_child():
    """`--labels`: pickled (X, min_cluster_size, min_samples) on stdin -> pickled labels on stdout, until stdin ends."""
    import pickle
    from numpy._core._multiarray_umath import __cpu_features__ as feat
    assert not feat['AVX2'] and not feat['AVX512_SKX'], 'numpy still dispatches a SIMD argsort: set NPY_DISABLE_CPU_FEATURES'
    from fuzz_hdbscan_vs_sklearn import sk_labels         # the one driver of scikit-learn's HDBSCAN (it needs the environment above)
    out = sys.stdout.buffer
    sys.stdout = sys.stderr
    while True:
        try:
            X, mcs, ms = pickle.load(sys.stdin.buffer)
        except EOFError:
            return
        pickle.dump(sk_labels(X, mcs, ms), out)
        out.flush()


class LabelsChild:
    def __init__(self):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--labels'], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  env=dict(os.environ, NPY_DISABLE_CPU_FEATURES=DISABLE))

    def __call__(self, X, mcs, ms):
        import pickle
        pickle.dump((X, mcs, ms), self.p.stdin)
        self.p.stdin.flush()
        return pickle.load(self.p.stdout)

    def close(self):
        self.p.stdin.close()
        self.p.wait()


class ProxyHDBSCAN:
    """In the place of hdbscan.HDBSCAN: keeps the keywords it is constructed with; fit_predict answers with scikit-learn's labels."""
    made = []           # keywords of every construction
    findings = []       # X on which the oracle's labels differ from scikit-learn's
    child = None        # LabelsChild (setup)

    def __init__(self, **kw):
        self.kw = dict(kw)
        self.last = None
        ProxyHDBSCAN.made.append(self.kw)

    def fit_predict(self, X):
        X = np.array(X, np.int64, copy=True)
        assert len(X) <= MAX_POINTS + 1500, len(X)
        labels = ProxyHDBSCAN.child(X, self.kw['min_cluster_size'], self.kw['min_samples'])
        if not np.array_equal(labels, H.hdbscan_labels(X, self.kw['min_cluster_size'], self.kw['min_samples'])):
            ProxyHDBSCAN.findings.append(X)
        self.last = (X, labels.copy())
        return labels


class HandLabels:
    """Part B's clusterer: hands out the label vector it was given, once."""

    def __init__(self, labels):
        self.labels, self.seen = labels, None

    def fit_predict(self, X):
        assert self.seen is None and self.labels is not None and len(X) == len(self.labels)
        self.seen = np.array(X, np.int64, copy=True)
        return np.asarray(self.labels, np.int64).copy()


# ---- part A: the videos ---------------------------------------------------------------------------------------------------------
def _seg_sel(fc, cuts, skip=6, read_batch=2000):
    trans = [0] + list(cuts) + [fc]
    true_inds, m2o, _ = P.select_frames(fc, fc, trans, skip, read_batch)
    seg = P.scenes_from_trans_inds(trans, fc)
    return len(true_inds), [m2o[int(s[0])] for s in seg]


def find_cuts(fc, wanted):
    """Frames at which scenes must start so that they start at the wanted SELECTED indices (used to place the cuts only: what the
    fixture records is the reference's own segmentation_sel, and the census is taken from what its calls received)."""
    cuts = []
    for wv in wanted:
        for c in (range((cuts[-1] + 1) if cuts else 1, fc - 1) if wv >= 0 else range(fc - 2, 0, -1)):
            n, starts = _seg_sel(fc, cuts + [c])
            if len(starts) == len(cuts) + 2 and starts[-1] == (wv if wv >= 0 else n + wv) and len(set(starts)) == len(starts):
                cuts.append(c)
                break
        else:
            raise RuntimeError('no frame starts a scene at selected index %d of %d frames' % (wv, fc))
    return cuts


def case_spec(i):
    rng = np.random.RandomState(3000 + i)
    family, wanted = FAMILIES[i % len(FAMILIES)]
    set_name = list(SETS)[i % len(SETS)]
    if i in SQUARE:
        w, h, fc = 720, 720, SQUARE[i]
    else:
        (w, h), fc = SIZES[i % 2], int(rng.randint(70, 151))
    if i >= len(FAMILIES) and family == 'no_cut':
        family, wanted = 'random_cuts', sorted(set(int(v) for v in rng.randint(3, 9, 2)))
    cuts = find_cuts(fc, wanted)
    best, over = SETS[set_name]
    over = dict(over, clust_filt=True, out_ratio=G.RATIOS[(2 * i + i // 5) % len(G.RATIOS)])
    return dict(index=i, family=family, set=set_name, best=best, overrides=over, w=w, h=h, fr=G.FRS[(3 * i + i // 5) % len(G.FRS)],
                fc=fc, trans_inds=[0] + cuts + [fc], empty=None)


KINDS = ('eq2', 'eq3_out', 'bright_small', 'eq4', 'eq2_out', 'eq_weak', 'eq3', 'eq4_out', 'single')


def _cells(rng, hp, wp):
    ny, nx = max(2, hp // 46), max(2, wp // 46)
    cells = [(int((r + 0.5) * hp / ny), int((c + 0.5) * wp / nx)) for r in range(ny) for c in range(nx)]
    rng.shuffle(cells)
    return cells


def _design_map(m, kind, rng, t_thr, tags):
    """One prepared map: flat nested rectangles (G._blob) in shuffled cells of the map."""
    hp, wp = m.shape
    cells = _cells(rng, hp, wp)
    jit = lambda: int(rng.randint(-5, 6))                # noqa: E731
    size = lambda: (int(rng.randint(4, 9)), int(rng.randint(4, 9)))      # noqa: E731
    v = int(rng.randint(t_thr + 40, 256))
    if kind.startswith('eq'):                             # blobs of EQUAL peak and different sizes: their maxima tie by construction
        n_eq = int(kind[2]) if kind[2].isdigit() else int(rng.randint(2, 4))
        for cy, cx in cells[:n_eq]:
            a, b = size()
            G._blob(m, cx + jit(), cy + jit(), a, b, v)
        if kind == 'eq_weak':                             # ... plus one smaller, weaker blob
            cy, cx = cells[n_eq]
            G._blob(m, cx + jit(), cy + jit(), 3, 3, v - 8)
        used = n_eq + 1
    elif kind == 'bright_small':                          # the brightest is not the largest: maximum and sum disagree
        cy, cx = cells[0]
        G._blob(m, cx + jit(), cy + jit(), 4, 4, v)
        for j, (cy, cx) in enumerate(cells[1:int(rng.randint(3, 5))]):
            G._blob(m, cx + jit(), cy + jit(), 8 - j, 8, v - 5 - 4 * j)
        used = 4
    else:
        cy, cx = cells[0]
        a, b = size()
        G._blob(m, cx + jit(), cy + jit(), a, b, v)
        used = 1
    if kind.endswith('_out'):                             # sparse outliers at a lower level: noise, which the filter must zero
        for cy, cx in cells[used:used + 3]:
            m[cy + jit(), cx + jit()] = t_thr + int(rng.randint(0, 10))
    tags.add(kind)


def _clump(m, count, y0, x0, level):
    """Exactly `count` points: rows of six from (y0, x0) on."""
    for k in range(count):
        m[y0 + k // 6, x0 + k % 6] = level


def design_maps(spec, rng, true_inds, seg_sel, hp, wp):
    """One prepared map per selected frame.  Blend chains (runs of maps next to a scene start, :2369-2370) get maps of two or more
    blobs, so that the filter removes points before every blend; the directed families put empty maps, the two point-count gates
    and a pair whose blend wraps in uint8 where their name says."""
    n = len(true_inds)
    tags = set()
    t_thr = 90 if spec['best'] else 120
    hmin = 5 if spec['best'] else 26
    maps = np.zeros((n, hp, wp), np.uint8)
    starts = sorted(int(s[0]) for s in seg_sel)
    near = lambda k: any(abs(k - s) <= 1 for s in starts)     # noqa: E731
    multi = [k for k in KINDS if k != 'single']
    off = spec['index']
    for k in range(n):
        kind = KINDS[(k + off) % len(KINDS)]
        if near(k) and kind == 'single':
            kind = multi[(k + off) % len(multi)]
        _design_map(maps[k], kind, rng, t_thr, tags)
    fam = spec['family']
    s = starts[-1]
    if fam == 'empty_chain_start':
        maps[s - 1] = 0
    elif fam == 'empty_chain_middle':
        maps[s] = 0
    elif fam == 'empty_chain_end':
        maps[s + 2] = 0
    elif fam == 'gates':                                   # N = hdbscan_min + 1 (not clustered) and + 2 (clustered), on maps no blend reaches
        free = [k for k in range(2, n - 1) if not near(k) and not near(k - 1)]
        for k, count in zip(free[:2], (hmin + 1, hmin + 2)):
            maps[k] = 0
            _clump(maps[k], count - 3, hp // 3, wp // 3, 200)
            _clump(maps[k], 3, hp // 3 + 20, wp // 3 + 30, 180)
        tags.add('gates')
    elif fam == 'wrap':                                    # 200 kept in map k, 100 (130 above the default threshold) under it in map k + 1
        low = 100 if spec['best'] else 130
        for k in (0, s):
            maps[k:k + 2] = 0
            cy, cx = hp // 2 + int(rng.randint(-9, 10)), wp // 2 + int(rng.randint(-9, 10))
            maps[k, cy - 6:cy + 7, cx - 6:cx + 7] = 200
            maps[k, 8:14, 8:16] = 150
            maps[k + 1, cy - 3:cy + 10, cx - 3:cx + 10] = low
            G._blob(maps[k + 1], wp - 20, hp - 20, 6, 6, 180)
        tags.add('wrap_pair')
    assert int((maps >= t_thr).reshape(n, -1).sum(1).max()) <= MAX_POINTS
    return maps, tags


def hooks(R, rec):
    rec.update(calls_in=[], calls_out=[], fits=[], ctor=None)

    def before(clusterer, sal_map, CP, *a, **k):
        rec['calls_in'].append(np.array(sal_map, np.uint8, copy=True))
        clusterer.last = None
        rec['ctor'] = dict(clusterer.kw)

    def after(r, clusterer, sal_map, CP, *a, **k):
        rec['calls_out'].append(np.array(r, np.uint8, copy=True))
        rec['fits'].append(clusterer.last)

    def loop_done(VD, *a, **k):
        rec['after'] = np.ascontiguousarray(np.transpose(VD['smaps'], (2, 0, 1))).copy()
    R.wrap('sc_clustering_filt', before=before, after=after)
    R.wrap('sc_handle_empty_centers', before=loop_done)


def generate_case(ref, stubs, i):
    """Case i with the first seed (7000 + 100 i + attempt; the fixture keeps it) on which the reference runs through and no frame is
    ambiguous.  rec['rejected']: [(seed, why)] of the seeds passed over, printed by main and reported in the notes."""
    spec = case_spec(i)
    rejected = []
    for attempt in range(20):
        seed = 7000 + 100 * i + attempt
        try:
            rec = G.run_case(ref, stubs, spec, seed, design=design_maps, hooks=hooks)
        except (TypeError, IndexError, ValueError) as e:     # the reference itself fails on these maps
            rejected.append((seed, 'the reference raised %s: %s' % (type(e).__name__, e)))
            continue
        if not rec['ambiguous'].any():
            rec['rejected'] = rejected
            return rec
        rejected.append((seed, 'ambiguous %d of %d frames' % (rec['ambiguous'].sum(), rec['fc'])))
    raise RuntimeError('case %d: no seed gives a usable video (%s)' % (i, rejected))


# ---- part B ---------------------------------------------------------------------------------------------------------------------
def part_b_cases():
    """-> [(name, map u8 [h, w], labels or None, CP overrides)].  A map is a list of rectangles (y0, y1, x0, x1, level, label);
    labels follow the points in raster order."""
    rng = np.random.RandomState(99)
    out = []

    def build(h, w, rects, name, **over):
        m = np.zeros((h, w), np.uint8)
        lab = np.full((h, w), -2, np.int64)
        for y0, y1, x0, x1, level, label in rects:
            m[y0:y1, x0:x1] = level
            lab[y0:y1, x0:x1] = label
        out.append((name, m, lab[m > 0].copy(), dict(over)))

    def row(h, w, k):
        """k rectangles in raster order of their first point, of different sizes."""
        ys = np.linspace(2, h - 12, k).astype(int)
        xs = rng.permutation(np.linspace(2, w - 14, k).astype(int))
        wd = max(5, (w - 16) // (k - 1))                     # (narrower than the columns are apart: no two overlap)
        return [(int(y), int(y) + int(rng.randint(4, 9)), int(x), int(x) + int(rng.randint(4, wd))) for y, x in zip(ys, xs)]

    shapes = [(24, 40), (36, 55), (48, 70), (60, 90)]
    si = 0
    for k in (2, 3, 4):                                       # k clusters, all tied at the top level; the label order is a permutation
        for where in ('first', 'middle', 'last'):            # of the raster order: the winner (label 0) lies first, in the middle, last
            for ss in (0, 1, 2, 3):
                h, w = shapes[si % 4]
                si += 1
                r = row(h, w, k)
                pos = dict(first=0, middle=k // 2, last=k - 1)[where]
                order = [pos] + [j for j in range(k) if j != pos]       # label -> rectangle
                label_of = {rect: lab for lab, rect in enumerate(order)}
                if ss == 1:                                   # equal SUMS: equal areas and levels
                    r = [(y0, y0 + 5, x0, x0 + 6) for (y0, y1, x0, x1) in r]
                rects = [r[j] + (200, label_of[j]) for j in range(k)]
                build(h, w, rects, 'tie%d_winner_%s_ss%d' % (k, where, ss), select_sum=ss, hdbscan_min=5)
    h, w = 36, 55                                             # label 0 loses: to a later maximum, to a later sum
    build(h, w, [(2, 8, 2, 12, 150, 0), (12, 18, 20, 30, 220, 1), (24, 30, 40, 50, 220, 2)], 'label0_loses_max', select_sum=2, hdbscan_min=5)
    build(h, w, [(2, 6, 2, 8, 250, 0), (12, 22, 20, 40, 130, 1), (26, 30, 44, 50, 250, 2)], 'label0_loses_sum', select_sum=1, hdbscan_min=5)
    build(h, w, [(2, 6, 2, 8, 250, 0), (12, 22, 20, 40, 130, 1), (26, 30, 44, 50, 240, 2)], 'brightest_is_label0_max', select_sum=0, hdbscan_min=5)
    build(h, w, [(2, 8, 2, 12, 150, -1), (12, 18, 20, 30, 220, -1)], 'all_noise', select_sum=2, hdbscan_min=5)
    build(h, w, [(2, 8, 2, 12, 150, 0)], 'one_cluster_no_noise', select_sum=2, hdbscan_min=5)
    build(h, w, [(2, 8, 2, 12, 150, 0), (20, 21, 30, 33, 250, -1), (30, 31, 5, 6, 255, -1)], 'one_cluster_bright_noise', select_sum=2, hdbscan_min=5)
    build(h, w, [(2, 8, 2, 12, 150, 1), (12, 18, 20, 30, 220, 0), (24, 30, 40, 50, 130, -1)], 'noise_and_two', select_sum=1, hdbscan_min=5)
    out.append(('empty', np.zeros((24, 40), np.uint8), None, dict(select_sum=2, hdbscan_min=5)))
    for hmin in (5, 26):                                      # the gate: N = hdbscan_min + 1 is not clustered, + 2 is
        for extra in (1, 2):
            m = np.zeros((30, 44), np.uint8)
            _clump(m, hmin + extra - 2, 4, 4, 200)
            _clump(m, 2, 20, 30, 140)
            n = hmin + extra
            lab = None if extra == 1 else np.array([0] * (n - 2) + [-1, -1], np.int64)
            out.append(('gate_min%d_plus%d' % (hmin, extra), m, lab, dict(select_sum=2, hdbscan_min=hmin)))
    # a sum past 2**16: 400 points of 255 (102 000; 36 464 modulo 2**16) against 200 points of 250 (50 000)
    build(60, 90, [(2, 22, 2, 22, 255, 1), (30, 40, 40, 60, 250, 0)], 'sum_past_2_16', select_sum=1, hdbscan_min=26)
    build(60, 90, [(2, 22, 2, 22, 255, 0), (30, 40, 40, 60, 250, 1)], 'sum_past_2_16_label0', select_sum=1, hdbscan_min=26)
    return out


def run_part_b(ref):
    recs = []
    for name, m, lab, over in part_b_cases():
        CP = ref.sc_init_crop_params(use_best_settings=False)
        CP.update(FIX)
        CP.update(over)
        cl = HandLabels(lab)
        got = ref.sc_clustering_filt(cl, m.copy(), CP)
        assert (cl.seen is not None) == (lab is not None), name
        if lab is not None:
            assert np.array_equal(cl.seen, np.argwhere(m > 0)), name
        recs.append(dict(name=name, map=m, out=np.array(got, np.uint8, copy=True), labels=lab, over=over))
    return recs


# ---- the file -------------------------------------------------------------------------------------------------------------------
def _labels_of(rec):
    return [None if f is None else f[1] for f in rec['fits']]


def pack(recs, brecs):
    empty_iou = (np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32), np.zeros(0, np.float64))
    out = G.pack(recs, empty_iou)
    for k in ('iou_a', 'iou_b', 'iou'):
        del out[k]
    n_in, in_idx, in_maps, nfit, labels = [], [], [], [], []
    for r in recs:
        n = r['fc_sel']
        assert len(r['calls_in']) == len(r['calls_out']) == len(r['fits']) == n
        diff = [i for i in range(n) if not np.array_equal(r['calls_in'][i], r['thr'][i])]
        n_in.append(len(diff))
        in_idx += diff
        in_maps += [r['calls_in'][i].reshape(-1) for i in diff]
        for i, f in enumerate(r['fits']):
            if f is not None:
                assert np.array_equal(f[0], np.argwhere(r['calls_in'][i] > 0))       # X is the raster-order point list of the map
                assert f[1].min() >= -1 and f[1].max() < 32767
            nfit.append(-1 if f is None else len(f[1]))
            if f is not None:
                labels.append(f[1].astype(np.int16))
    cat = lambda seq, dt: np.concatenate(seq).astype(dt) if len(seq) else np.zeros(0, dt)      # noqa: E731
    out['n_filt_in'] = np.asarray(n_in, np.int32)
    out['filt_in_idx'] = np.asarray(in_idx, np.int32)
    out['filt_in_maps'] = cat(in_maps, np.uint8)
    out['filt_out'] = np.concatenate([np.stack(r['calls_out']).reshape(-1) for r in recs])
    out['after'] = np.concatenate([r['after'].reshape(-1) for r in recs])
    out['nfit'] = np.asarray(nfit, np.int32)
    out['labels'] = cat(labels, np.int16)
    out['ctor'] = np.asarray([json.dumps(r['ctor'], sort_keys=True) for r in recs])
    out['b_name'] = np.asarray([b['name'] for b in brecs])
    out['b_shape'] = np.asarray([b['map'].shape for b in brecs], np.int32)
    out['b_map'] = np.concatenate([b['map'].reshape(-1) for b in brecs])
    out['b_out'] = np.concatenate([b['out'].reshape(-1) for b in brecs])
    out['b_nfit'] = np.asarray([-1 if b['labels'] is None else len(b['labels']) for b in brecs], np.int32)
    out['b_labels'] = cat([b['labels'] for b in brecs if b['labels'] is not None], np.int16)
    out['b_over'] = np.asarray([json.dumps(b['over'], sort_keys=True) for b in brecs])
    return out


def census_view(ref, rec):
    CP = ref.sc_init_crop_params(use_best_settings=rec['spec']['best'])
    CP.update(rec['spec']['overrides'])
    return dict(CP=CP, fc=rec['fc'], fc_sel=rec['fc_sel'], thr=rec['thr'], calls_in=rec['calls_in'], calls_out=rec['calls_out'],
                labels=_labels_of(rec), segmentation_sel=rec['segmentation_sel'])


def setup(ref_dir):
    ref = load_reference(ref_dir)
    stubs = G.Stubs(ref)
    ref.hdbscan.HDBSCAN = ProxyHDBSCAN
    if ProxyHDBSCAN.child is None:
        import atexit
        ProxyHDBSCAN.child = LabelsChild()
        atexit.register(ProxyHDBSCAN.child.close)
    return ref, stubs


def main():
    if sys.argv[1:] == ['--labels']:
        return labels_child()
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref, stubs = setup(sys.argv[1])
    recs = [generate_case(ref, stubs, i) for i in range(N_CASES)]
    if ProxyHDBSCAN.findings:
        sys.exit('FINDING: oracle.hdbscan_ref differs from scikit-learn on %d point sets (first: N = %d)'
                 % (len(ProxyHDBSCAN.findings), len(ProxyHDBSCAN.findings[0])))
    for r in recs:
        assert r['fc_sel'] <= 32 and max(r['h_process'], r['w_process']) <= 250 and not r['scattered']
        assert np.array_equal(r['after'], np.stack(r['calls_out']))          # (:2364: the returned map IS map i after the loop)
    for r in recs:
        for seed, why in r['rejected']:
            print('case %d: seed %d passed over (%s)' % (r['spec']['index'], seed, why))
    print('%d seeds passed over in %d of %d cases' % (sum(len(r['rejected']) for r in recs), sum(bool(r['rejected']) for r in recs), len(recs)))
    z = RCC.census([census_view(ref, r) for r in recs])
    print(json.dumps(z))
    short = {k: (z[k], v) for k, v in CAPS.items() if z[k] < v}
    if short or not z['gate_plus1'] or not z['gate_plus2'] or not z['noise_zeroed']:
        sys.exit('the census misses its caps (have, want): %s' % short)
    brecs = run_part_b(ref)
    out = pack(recs, brecs)
    out['crop_params'] = G.crop_params_of(ref)
    path = os.path.join(os.path.dirname(_TOOLS), 'tests', 'golden', 'refpath_clustered_golden.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('%s: %d videos, %d frames, %d selected, %d direct calls, %d bytes' % (path, len(recs), z['frames'], z['selected'], len(brecs), size))
    if size > G.SIZE_LIMIT:
        sys.exit('the fixture is larger than %d bytes' % G.SIZE_LIMIT)


if __name__ == '__main__':
    main()
