"""-m gpu: every run-time path of the tail (k_core's phases and forms, k_tree_par's modes and its hand-over to k_tree, k_tree's
forms) taken on purpose and judged by the oracle.

Each map is built for one path (tests/tail_paths.py; tests/test_tail_paths_host.py shows on the CPU that it lies there).  Here
the default engine runs it and two things are checked: PATH -- the frame header (the k_core stamps, HDR_TREE_PAR, HDR_NCLUSTERS,
HDR_BACK_DONE) agrees with the predictor -- and RESULT -- point list, core distances, Prim edge list, labels up to renaming, final
map and centre are the oracle's.  Maps too large for the oracle's O(N^2) in a test's seconds have their core distances checked
against the oracle's brute force and everything else against the reference engine (ops.tail_engine(reference=True)), which the
last test checks against the oracle at k_tree's own seams."""
import numpy as np
import pytest
import torch

import tail_paths as tp
from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import hdbscan_ref as H
from retargetvid_amd import ops
from test_gpu_parity import _check_tail

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]


def _plan(engine, shape, CP):
    """The engine's plan for the shape, which is also the fixture's: the host test placed the cases by the same numbers."""
    plan = engine.tail_plan(shape[0], shape[1], CP)
    assert plan == tp.default_plan(shape[0], shape[1], CP)
    return plan


def _state_is_the_oracles(engine, i, clustered, CP):
    """test_gpu_parity._state_is_the_oracles on the oracle run the predictor has made already: point list, core distances, Prim
    edge list, labels up to renaming -> (state, oracle)."""
    st = engine.cluster_state(i, clustered.size)
    X = np.stack([st['pts'] & 255, (st['pts'] >> 8) & 255], 1).astype(np.int64)
    assert np.array_equal(X, np.argwhere(clustered > 0)), i
    if len(X) <= CP['hdbscan_min'] + 1:
        return st, None
    o = tp.oracle_hdbscan(clustered, CP)
    assert np.array_equal(o['core'], st['core']), i
    assert np.array_equal(o['mst'], st['mst']), 'Prim sequence of map %d (N = %d)' % (i, len(X))
    ref, got = o['labels'], st['labels']
    assert np.array_equal(ref < 0, got < 0), i
    pairs = {(a, b) for a, b in zip(ref[ref >= 0], got[got >= 0])}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}), 'labels of map %d' % i
    return st, o


def _path_and_result(engine, maps, flags, CP, plan, reference=False):
    """One call on raw maps: final maps and centres against the oracle's (_check_tail), then per map the state against the
    oracle's and the header against the predictor -> [(state, core prediction, hierarchy prediction)]."""
    seen, final, dx, dy = tp.blended_inputs(maps, flags, CP)
    _check_tail(engine, maps, flags, CP, (final, dx, dy, None))
    out = []
    for i in range(len(maps)):
        st, o = _state_is_the_oracles(engine, i, seen[i], CP)
        core = tp.predict_core(seen[i], CP, plan)
        hier = tp.predict_hierarchy(core['N'], o['nclusters'], CP, plan, reference) if o is not None else None
        bad = tp.header_agrees(st['hdr'], core, hier, o['nclusters'] if o is not None else None)
        assert not bad, (i, bad)
        out.append((st, core, hier))
    return out


def test_the_plan_fixture_is_the_doors(engine):
    """tests/golden/tail_plan.json (what the host tests place their cases by) equals the door, word for word; the reference engine
    plans one launch per stage with k_tree behind; the door refuses what svc_cluster_center refuses."""
    from retargetvid_amd._lib import SvcError
    fx = tp._fixture()
    assert fx['words'] == list(ops.TAIL_PLAN_WORDS)
    for key, (h, w, CP) in tp.fixture_requests().items():
        assert engine.tail_plan(h, w, CP) == fx['plans'][key], key
    best = engine.tail_plan(140, 250, tp.P.init_crop_params(True))             # the shape the tail clusters on: shrunk by 4
    assert (best['h'], best['w']) == (35, 62)
    ref = ops.tail_engine(reference=True)
    try:
        plan = ref.tail_plan(140, 250, tp.DEFAULT)
        assert (plan['fused'], plan['tree_fallback']) == (0, 1)
        assert {k: v for k, v in plan.items() if k not in ('fused', 'lvl_big')} == {k: v for k, v in fx['plans']['140x250/26'].items() if k not in ('fused', 'lvl_big')}
    finally:
        ref.close()
    for h, w, CP, text in ((300, 300, tp.DEFAULT, 'exceeds the supported'), (140, 250, dict(tp.DEFAULT, hdbscan_min=1), 'hdbscan_min'),
                           (7, 250, dict(tp.DEFAULT, resize_factor=16), 'too small')):
        with pytest.raises(SvcError, match=text):
            engine.tail_plan(h, w, CP)


@pytest.mark.parametrize('kname', list(tp.K_SETS))
def test_k_core_directed_maps(engine, kname):
    """Phases 1 and 2 with the k-th hit on a chosen slot of the ring table (the last distance of the phase, the last slot of a
    group of eight and the first of the next, the last lane of a ballot and the first of the next, across a 256-offset step), at
    an interior point, beside every border and in every corner; phase 3's answer at its lower bound, at the gallop's first probe
    and just above it.  One call per k: k = 26, 3, 1 and N - 1."""
    CP = tp.K_SETS[kname]
    plan = _plan(engine, tp.DIRECTED_SHAPE, CP)
    ring = tp.ring_of(plan)
    cases = [(label, m, at, 1, int(ring[idx, 2])) for label, m, at, idx in tp.phase1_cases(kname, plan)]
    cases += [(label, m, at, 2, int(ring[idx, 2])) for label, m, at, idx in tp.phase2_cases(kname, plan)]
    cases += [(label, m, at, 3, d2) for label, m, at, d2 in tp.answer_cases(kname, plan)]
    maps = np.stack([c[1] for c in cases])
    got = _path_and_result(engine, maps, None, CP, plan)
    for (label, m, (r, c), phase, d2), (st, core, hier) in zip(cases, got):
        p = tp.point_index(m, r, c)
        assert core['phase'][p] == phase and st['core'][p] == d2, label
        assert hier['tree_par'] == 1, label


def test_k_core_answer_at_the_maps_diagonal(engine):
    """Two points in opposite corners, k = N - 1: the answer is phase 3's upper bound, which the gallop never probes."""
    plan = _plan(engine, tp.DIRECTED_SHAPE, tp.DIAGONAL_CP)
    m, diag = tp.diagonal_case(tp.DIRECTED_SHAPE)
    (st, core, hier), = _path_and_result(engine, m[None], None, tp.DIAGONAL_CP, plan)
    assert core['counts'][3] == 4 and st['core'][0] == st['core'][3] == diag


@pytest.mark.parametrize('kname', list(tp.K_SETS))
def test_k_core_phase_3_register_forms_and_the_lds_loop(engine, kname):
    """Maps of 512 / 513, 1024 / 1025, 1536 / 1537 and 2048 / 2049 points (the last size of every register form and the first
    of the next; 2 049: the LDS loop), one point of each alone in a hole wider than the ring table; with k = N - 1 every point
    takes phase 3."""
    CP = tp.K_SETS[kname]
    plan = _plan(engine, tp.HOLE_SHAPE, CP)
    cases = tp.hole_cases(kname, plan)
    got = _path_and_result(engine, np.stack([c[1] for c in cases]), None, CP, plan)
    for (label, m, (r, c), form), (st, core, hier) in zip(cases, got):
        assert core['phase3_form'] == form and core['phase'][tp.point_index(m, r, c)] == 3, label


def _equal_the_reference_engines(engine, ref, maps, flags, CP, cap):
    """The default engine's maps, stats, centres, Prim edge lists and labels against the reference engine's -> (states, reference states)."""
    a, b = torch.from_numpy(maps).cuda(), torch.from_numpy(maps).cuda()
    xa, sa = ref.cluster_center_(a, flags, CP, want_stats=True)
    xb, sb = engine.cluster_center_(b, flags, CP, want_stats=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert np.array_equal(xa.cpu().numpy(), xb.cpu().numpy(), equal_nan=True)
    olds, news = [], []
    for i in range(len(maps)):
        s_old, s_new = ref.cluster_state(i, cap), engine.cluster_state(i, cap)
        assert np.array_equal(s_old['pts'], s_new['pts']) and np.array_equal(s_old['core'], s_new['core']), i
        assert np.array_equal(s_old['mst'], s_new['mst']), 'Prim sequence of map %d (N = %d)' % (i, s_old['n'])
        assert np.array_equal(s_old['labels'], s_new['labels']), 'labels of map %d' % i
        assert s_old['hdr'][ops.HDR_NCLUSTERS] == s_new['hdr'][ops.HDR_NCLUSTERS], i
        olds.append(s_old)
        news.append(s_new)
    return news, olds


def test_k_core_phase_3_lds_and_global_loops(engine):
    """A dense 96 x 96 map with one point alone in a hole, at the largest N that keeps the points in LDS and one point more (the
    global loop), k = 26; the second map again with hdbscan_min_samples above the ring table's size, so that every point takes
    the global loop.  Core distances against the oracle's brute force; the rest against the reference engine."""
    plan = _plan(engine, tp.GLOBAL_SHAPE, tp.DEFAULT)
    maps, (r, c) = tp.loop_maps(plan)
    ref = ops.tail_engine(reference=True)
    try:
        for CP, which in ((tp.DEFAULT, (0, 1)), (dict(tp.DEFAULT, hdbscan_min_samples=plan['n_ring'] + 1), (1,))):
            sub = maps[list(which)]
            news, _ = _equal_the_reference_engines(engine, ref, sub, None, CP, maps[0].size)
            for m, st in zip(sub, news):
                core = tp.predict_core(m, CP, plan)
                assert core['phase3_form'] == ('global' if core['N'] > plan['core_lds_max'] else 'lds')
                assert core['phase'][tp.point_index(m, r, c)] == 3
                if CP['hdbscan_min_samples']:
                    assert core['counts'][3] == core['N']
                assert not tp.header_agrees(st['hdr'], core)
                X = np.argwhere(m > 0)
                assert np.array_equal(X, np.stack([st['pts'] & 255, (st['pts'] >> 8) & 255], 1))
                assert np.array_equal(H.core_distances(X, core['k']), st['core'])
    finally:
        ref.close()


def test_the_seam_between_k_tree_pars_modes_at_tp_cap_points(engine):
    """TP_CAP - 1, TP_CAP and TP_CAP + 1 points in ONE call (72 x 72 noise), with and without cut-blend flags, both parameter
    sets, against the reference engine; in every call the header agrees with the predictor on what the cluster filter saw
    (a blended map is another map: under the best-like set it grows past the tables and is handed over); without flags
    k_tree_par keeps all three (HDR_TREE_PAR), and the TP_CAP + 1 map is the oracle's."""
    ref = ops.tail_engine(reference=True)
    try:
        for CP in (tp.DEFAULT, tp.BEST_LIKE):
            plan = _plan(engine, tp.SEAM_SHAPE, CP)
            maps = tp.point_seam_maps(plan)
            for flags in (np.array([1, 1, 0], np.uint8), None):
                news, _ = _equal_the_reference_engines(engine, ref, maps, flags, CP, maps[0].size)
                seen = tp.blended_inputs(maps, flags, CP)[0]         # (with flags maps 1 and 2 are blends: other maps, other paths)
                for i, (m, st) in enumerate(zip(seen, news)):
                    o = tp.oracle_hdbscan(m, CP)
                    hier = tp.predict_hierarchy(st['n'], o['nclusters'], CP, plan)
                    assert not tp.header_agrees(st['hdr'], tp.predict_core(m, CP, plan), hier, o['nclusters']), (i, flags)
            assert [st['n'] for st in news] == [plan['TP_CAP'] - 1, plan['TP_CAP'], plan['TP_CAP'] + 1]
            assert all(st['hdr'][ops.HDR_TREE_PAR] == 1 and st['hdr'][ops.HDR_BACK_DONE] == 1 for st in news)
            _state_is_the_oracles(engine, 2, maps[2], CP)
    finally:
        ref.close()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_k_tree_pars_cluster_tables_at_the_cap_and_above(engine, mode):
    """Per mode of k_tree_par (N <= TP_CAP, <= TP_CAP_BIG, beyond: cap_cl_huge) two tile maps in one call: the largest cluster
    count the tables hold (the map is kept: HDR_TREE_PAR 1) and the next one a binary merge tree has (handed to k_tree and
    k_finish: 0).  HDR_NCLUSTERS, state, final maps and centres are the oracle's."""
    CP0 = tp.TABLE_SEAMS[mode][0]
    plan = _plan(engine, tp.FULL_SHAPE, CP0)
    CP, maps, tiles = tp.table_seam_maps(mode, plan)
    got = _path_and_result(engine, np.stack(maps), None, CP, plan)
    assert [h['tree_par'] for _, _, h in got] == [1, 0] and [h['mode'] for _, _, h in got] == [mode, mode]
    assert [st['hdr'][ops.HDR_NCLUSTERS] for st, _, _ in got] == [2 * t - 1 for t in tiles]


def test_kept_and_handed_over_maps_in_one_blend_chain(engine):
    """Maps that k_tail_back finishes and maps it hands to k_tree + k_finish alternate in one call, each blended into the
    next: HDR_BACK_DONE 1, 0, 1, 0; maps and centres are the oracle's."""
    plan = _plan(engine, tp.FULL_SHAPE, tp.TABLE_SEAMS[0][0])
    CP, maps, flags = tp.mixed_call_maps(plan)
    got = _path_and_result(engine, maps, flags, CP, plan)
    assert [st['hdr'][ops.HDR_BACK_DONE] for st, _, _ in got] == [1, 0, 1, 0]
    assert [st['hdr'][ops.HDR_TREE_PAR] for st, _, _ in got] == [1, 0, 1, 0]


def test_the_reference_engine_against_the_oracle_at_k_trees_seams():
    """k_tree itself (the reference engine: every map is its): TREE_LDS_CAP and TREE_LDS_CAP + 1 points (the LDS form's last map,
    the global form's first), and condensed clusters on both sides of TREE_LDS_CLUSTERS at few points (the LDS form, and its
    retry in global memory) -- state, HDR_NCLUSTERS, final maps and centres against the oracle."""
    ref = ops.tail_engine(reference=True)
    try:
        plan = tp.default_plan(*tp.SEAM_SHAPE, tp.DEFAULT)
        assert ref.tail_plan(*tp.SEAM_SHAPE, tp.DEFAULT)['TREE_LDS_CAP'] == plan['TREE_LDS_CAP']
        rng = np.random.RandomState(plan['TREE_LDS_CAP'])
        h, w = tp.SEAM_SHAPE
        maps = np.stack([tp.noise_map_with_n_points(rng, h, w, plan['TREE_LDS_CAP'] / float(h * w), n)
                         for n in (plan['TREE_LDS_CAP'], plan['TREE_LDS_CAP'] + 1)])
        got = _path_and_result(ref, maps, None, tp.DEFAULT, plan, reference=True)
        assert [hier['tree_form'] for _, _, hier in got] == ['lds', 'global']
        plan = tp.default_plan(*tp.FULL_SHAPE, tp.TABLE_SEAMS[0][0])
        CP, maps, tiles = tp.tree_cluster_seam_maps(plan)
        got = _path_and_result(ref, np.stack(maps), None, CP, plan, reference=True)
        assert [hier['tree_form'] for _, _, hier in got] == ['lds', 'lds_retry']
        assert [st['hdr'][ops.HDR_NCLUSTERS] for st, _, _ in got] == [2 * t - 1 for t in tiles]
        assert got[0][0]['hdr'][ops.HDR_NCLUSTERS] <= plan['TREE_LDS_CLUSTERS'] < got[1][0]['hdr'][ops.HDR_NCLUSTERS]
    finally:
        ref.close()
