"""No GPU: every directed map of tests/test_gpu_tail_paths.py lies on the path it is meant for, by the predictor of
tests/tail_paths.py and the default engine's plan (tests/golden/tail_plan.json: the words of the plan door as a GPU run read them;
the GPU test holds the file equal to the door).  And the census: which paths the maps of the existing tail tests reach."""
import os
import sys

import numpy as np
import pytest

import tail_paths as tp
from oracle import hdbscan_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree_path():
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'sim'))
    try:
        import tree_path
    finally:
        sys.path.pop(0)
    return tree_path


def test_the_fixture_holds_every_plan_the_cases_read():
    fx = tp._fixture()
    assert fx['engine'] == 'default' and set(fx['plans']) == set(tp.fixture_requests())
    from retargetvid_amd import ops
    assert fx['words'] == list(ops.TAIL_PLAN_WORDS)
    for key, plan in fx['plans'].items():
        assert sorted(plan) == sorted(ops.TAIL_PLAN_WORDS) and key == tp.plan_key(plan['h'], plan['w'], dict(hdbscan_min=int(key.split('/')[1])))
        assert plan['fused'] == 1 and len(tp.ring_of(plan)) == plan['n_ring']


def test_header_words_of_the_plan_door_are_the_bindings():
    """Every SVC_TAILPLAN_* of include/svc.h is a word of ops.TAIL_PLAN_WORDS at the same index (case aside)."""
    import re
    from retargetvid_amd import ops
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    words = {k: int(v) for k, v in re.findall(r'#define SVC_TAILPLAN_([A-Z0-9_]+)\s+(\d+)', text)}
    assert words.pop('WORDS') == len(ops.TAIL_PLAN_WORDS)
    assert {k.lower(): v for k, v in words.items()} == {w.lower(): i for i, w in enumerate(ops.TAIL_PLAN_WORDS)}


def test_the_cluster_count_is_births_plus_splits_of_the_path():
    """The predictor's condensed-cluster count (ids of the oracle's condensed tree) is what k_tree_par counts and both builders
    store in SVC_HDR_NCLUSTERS: the births and true splits of tools/sim/tree_path.py, on noise, blobs and tile maps."""
    S = _tree_path()
    rng = np.random.RandomState(5)
    ys, xs = np.mgrid[0:35, 0:62]
    maps = []
    for t in range(6):
        occ = rng.rand(35, 62) < (0.03, 0.1, 0.3)[t % 3]
        for _ in range(t % 3):
            occ |= ((ys - rng.uniform(5, 30)) ** 2 + (xs - rng.uniform(5, 55)) ** 2 < rng.uniform(10, 90))
        maps.append((occ * 200).astype(np.uint8))
    maps.append(tp.tile_map((35, 62), 40, 2, 3, 1))
    seen = set()
    for m in maps:
        for CP in (tp.BEST_LIKE, tp.K_SETS['k1'], dict(tp.DEFAULT, hdbscan_min=2, hdbscan_min_samples=1), tp.DEFAULT):
            o = tp.oracle_hdbscan(m, CP)
            u, v, w = o['mst'].T
            labels, nc = S.labels_path(u, v, w, H.edge_order(w), CP['hdbscan_min'], with_nc=True)
            assert S.same_partition(o['labels'], labels)
            assert nc == o['nclusters'] and nc % 2 == 1
            seen.add(nc)
    assert len(seen) > 8 and tp.oracle_hdbscan(maps[-1], tp.K_SETS['k1'])['nclusters'] == 2 * 40 - 1


def _target_paths(cases, CP, plan, phase):
    ring = tp.ring_of(plan)
    for label, m, (r, c), idx in cases:
        core = tp.predict_core(m, CP, plan)
        p = tp.point_index(m, r, c)
        assert core['clustered'] and core['k'] == (tp.K_OF[label.split('/')[0]]), label
        assert core['phase'][p] == phase and tp.kth_ring_index(m, r, c, core['k'], ring) == idx, label
        yield label, m, (r, c), idx, core, p


@pytest.mark.parametrize('kname', list(tp.K_SETS))
def test_directed_phase_1_and_2_maps_lie_on_their_paths(kname):
    CP = tp.K_SETS[kname]
    plan = tp.default_plan(*tp.DIRECTED_SHAPE, CP)
    ring, n1 = tp.ring_of(plan), plan['n_ring1']
    kinds = set()
    for label, m, (r, c), idx, core, p in _target_paths(tp.phase1_cases(kname, plan), CP, plan, 1):
        _, kind, pos = label.split('/')
        kinds.add((kind, pos))
        assert idx < n1 and core['interior'][p] == (pos == 'interior')
        if pos != 'interior':
            assert min(r, c, plan['h'] - 1 - r, plan['w'] - 1 - c) < plan['RING_R1']
        assert {'d16': ring[idx, 2] == plan['RING_R1'] ** 2, 'slot7': idx % 8 == 7, 'slot0': idx % 8 == 0 and idx >= 8}[kind], label
    # every kind at the interior point and at every border; in the corners wherever a corner's 16 offsets hold k hits
    assert {(kd, ps) for kd in tp.PHASE1_KINDS for ps in tp.POSITIONS[:5]} <= kinds
    assert (kname == 'k26') == (not any(ps in ('tl', 'tr', 'bl', 'br') for _, ps in kinds))
    if kname != 'k26':
        assert {ps for _, ps in kinds} == set(tp.POSITIONS) and len(kinds) >= 3 * 5 + 8
    kinds = set()
    for label, m, (r, c), idx, core, p in _target_paths(tp.phase2_cases(kname, plan), CP, plan, 2):
        _, kind, pos = label.split('/')
        kinds.add(kind)
        assert n1 <= idx < plan['n_ring']
        if kind == 'd17':
            assert ring[idx, 2] == plan['RING_R1'] ** 2 + 1
        elif kind.startswith('d400'):
            assert ring[idx, 2] == plan['RING_R'] ** 2 and tuple(ring[idx, :2]) == tuple(int(v) for v in kind.split('_')[1:])
        elif kind == 'corner':
            inb = tp._in_bounds(tp.DIRECTED_SHAPE, r, c, ring)
            assert (r in (0, plan['h'] - 1)) and (c in (0, plan['w'] - 1)) and inb.sum() * 4 < plan['n_ring'] + 4 * plan['RING_R'] + 4
            assert idx == np.nonzero(inb)[0][-1] and ring[idx, 2] == plan['RING_R'] ** 2
        else:                                   # last lane of a ballot, first lane of the next; the same across a 256-offset step
            assert idx == {'lane63': 63, 'lane0': 64, 'step255': 255, 'step256': 256}[kind] and idx % 64 in (63, 0)
    assert kinds == set(tp.PHASE2_KINDS) | {'corner'}


@pytest.mark.parametrize('kname', list(tp.K_SETS))
def test_directed_phase_3_maps_lie_on_their_paths(kname):
    CP = tp.K_SETS[kname]
    plan = tp.default_plan(*tp.DIRECTED_SHAPE, CP)
    lo = plan['RING_R'] ** 2 + 1
    want = {'lo': lo, 'twice_lo': 2 * lo}
    for label, m, (r, c), d2 in tp.answer_cases(kname, plan):
        core = tp.predict_core(m, CP, plan)
        p = tp.point_index(m, r, c)
        assert core['phase'][p] == 3 and core['phase3_form'] == 'regs8' and core['k'] == tp.K_OF[kname], label
        assert H.core_distances(np.argwhere(m > 0), core['k'])[p] == d2, label
        name = label.split('answer_')[1]
        assert d2 == want.get(name, d2) and (name != 'above_twice_lo' or (d2 > 2 * lo and tp.next_grid_distance(2 * lo)[0] == d2))
    plan = tp.default_plan(*tp.HOLE_SHAPE, CP)
    forms = []
    for label, m, (r, c), form in tp.hole_cases(kname, plan):
        core = tp.predict_core(m, CP, plan)
        assert core['phase'][tp.point_index(m, r, c)] == 3 and core['phase3_form'] == form, label
        assert core['k'] == (core['N'] - 1 if kname == 'kN' else tp.K_OF[kname])
        if kname == 'kN':
            assert core['counts'][3] == core['N']
        forms.append((core['N'], form))
    assert forms == [(512, 'regs8'), (513, 'regs16'), (1024, 'regs16'), (1025, 'regs24'), (1536, 'regs24'), (1537, 'regs32'),
                     (2048, 'regs32'), (2049, 'lds')] == list(zip(tp.register_form_counts(plan), [f for _, f in forms]))


def test_the_diagonal_and_the_loop_maps_lie_on_their_paths():
    plan = tp.default_plan(*tp.DIRECTED_SHAPE, tp.DIAGONAL_CP)
    m, diag = tp.diagonal_case(tp.DIRECTED_SHAPE)
    core = tp.predict_core(m, tp.DIAGONAL_CP, plan)
    assert core['N'] == 4 and core['k'] == 3 and core['counts'][3] == 4 and core['phase3_form'] == 'regs8'
    assert H.core_distances(np.argwhere(m > 0), 3)[[0, 3]].tolist() == [diag, diag] and diag == 71 ** 2 + 99 ** 2
    plan = tp.default_plan(*tp.GLOBAL_SHAPE, tp.DEFAULT)
    maps, (r, c) = tp.loop_maps(plan)
    for m, form in zip(maps, ('lds', 'global')):
        core = tp.predict_core(m, tp.DEFAULT, plan)
        assert core['phase'][tp.point_index(m, r, c)] == 3 and core['phase3_form'] == form and core['k'] == 26
        assert 0 < core['counts'][3] < 30                       # the isolated point and little else
    assert int((maps[1] > 0).sum()) == plan['core_lds_max'] + 1 == int((maps[0] > 0).sum()) + 1
    every = dict(tp.DEFAULT, hdbscan_min_samples=plan['n_ring'] + 1)
    core = tp.predict_core(maps[1], every, plan)
    assert core['counts'][3] == core['N'] and core['phase3_form'] == 'global'


def test_hierarchy_maps_lie_on_their_paths():
    # the point-count seam: k_tree_par's modes 0, 0, 1, every map kept, under both parameter sets
    for CP in (tp.DEFAULT, tp.BEST_LIKE):
        plan = tp.default_plan(*tp.SEAM_SHAPE, CP)
        got = []
        for m in tp.point_seam_maps(plan):
            o = tp.oracle_hdbscan(m, CP)
            got.append((len(o['X']), tp.predict_hierarchy(len(o['X']), o['nclusters'], CP, plan)))
        assert [n for n, _ in got] == [plan['TP_CAP'] - 1, plan['TP_CAP'], plan['TP_CAP'] + 1]
        assert [(h['mode'], h['tree_par']) for _, h in got] == [(0, 1), (0, 1), (1, 1)]
    # the cluster-table seam of every mode: the nearest reachable counts on either side of the cap
    for mode in (0, 1, 2):
        CP0 = tp.TABLE_SEAMS[mode][0]
        plan = tp.default_plan(*tp.FULL_SHAPE, CP0)
        CP, maps, tiles = tp.table_seam_maps(mode, plan)
        hs = []
        for m, t in zip(maps, tiles):
            o = tp.oracle_hdbscan(m, CP)
            assert o['nclusters'] == 2 * t - 1
            hs.append((o['nclusters'], tp.predict_hierarchy(len(o['X']), o['nclusters'], CP, plan)))
        cap = plan['cap_cl_huge'] if mode == 2 else plan['cap_cl']
        assert [h['mode'] for _, h in hs] == [mode, mode] and [h['cap'] for _, h in hs] == [cap, cap]
        assert cap - 1 <= hs[0][0] <= cap < hs[1][0] <= cap + 2
        assert [h['tree_par'] for _, h in hs] == [1, 0] and plan['tree_fallback'] == 1
    # the mixed call: kept, handed over, kept, handed over, in one blend chain
    plan = tp.default_plan(*tp.FULL_SHAPE, tp.TABLE_SEAMS[0][0])
    CP, maps, flags = tp.mixed_call_maps(plan)
    seen = tp.blended_inputs(maps, flags, CP)[0]
    hs = [tp.predict_hierarchy(len(o['X']), o['nclusters'], CP, plan) for o in (tp.oracle_hdbscan(m, CP) for m in seen)]
    assert [h['back_done'] for h in hs] == [1, 0, 1, 0] and flags.tolist() == [1, 1, 1, 0] and not np.array_equal(seen[1:], maps[1:])
    # k_tree's own seams (the reference engine): the LDS form's last point count, the global form; clusters around its tables
    plan = tp.default_plan(*tp.SEAM_SHAPE, tp.DEFAULT)
    assert plan['TREE_LDS_CAP'] in (plan['TP_CAP'] - 1, plan['TP_CAP'])          # (the point-seam maps serve both seams)
    forms = [tp.predict_hierarchy(int((m > 0).sum()), tp.oracle_hdbscan(m, tp.DEFAULT)['nclusters'], tp.DEFAULT, plan, reference=True)['tree_form']
             for m in tp.point_seam_maps(plan)]
    assert forms[-2:] == ['lds', 'global'] if plan['TREE_LDS_CAP'] == plan['TP_CAP'] else forms[:2] == ['lds', 'global']
    plan = tp.default_plan(*tp.FULL_SHAPE, tp.TABLE_SEAMS[0][0])
    CP, maps, tiles = tp.tree_cluster_seam_maps(plan)
    hs = [tp.predict_hierarchy(len(o['X']), o['nclusters'], CP, plan, reference=True) for o in (tp.oracle_hdbscan(m, CP) for m in maps)]
    assert [h['tree_form'] for h in hs] == ['lds', 'lds_retry'] and [h['tree_par'] for h in hs] == [0, 0]


def test_census_of_the_existing_tail_maps(capsys):
    """Which paths the maps of the existing tail tests reach (DESIGN.md holds the table).  What had no map before the directed
    tests: phase 3's global loop, a point count at TP_CAP, a cluster count at the tables' capacity."""
    entries = tp.existing_maps()
    counts, n_clustered, n_counted = tp.census(entries)
    with capsys.disabled():
        print('\ncensus: %d maps of the existing tail tests, %d clustered, %d with a cluster count (N <= %d)'
              % (len(entries), n_clustered, n_counted, tp.CENSUS_ORACLE_N))
        for path in tp.CENSUS_PATHS:
            print('  %-62s %4d' % (path, counts[path]))
    assert len(entries) > 400 and n_counted > 300
    assert counts['k_core phase 3: global'] == 0 and counts['N within 1 of TP_CAP'] == 0 and counts['clusters within 2 of the cap'] == 0
