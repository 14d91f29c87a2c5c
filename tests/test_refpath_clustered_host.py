"""The clustered crop path pinned to the reference's OWN code: tests/golden/refpath_clustered_golden.npz holds what the reference's
smart_vid_crop (smartVidCrop.py:2218-2614, clust_filt = True, op_close = False, resize_factor = 1) held around every call of its
sc_clustering_filt (:1062-1161) and behind its clustering loop (:2359-2373) on 24 videos, and what sc_clustering_filt returned
for ~50 hand-made label vectors (tools/make_golden_refpath_clustered.py; read back by tests/refpath_clustered_cases.py).  The
labels the reference was handed are scikit-learn's (the project's proxy for the hdbscan package) or made by hand: they are input
data here, never "the reference".  No GPU.

  census and caps        asserted on the fixture: ties, the sum rule, blend chains, wraps, the `<` of i < fc_sel - 2, the gates
  glue                   tail_ref.clustering_filt with the recorded labels replayed = the reference's returned map, every call of
                         both parts, byte for byte; the constructor keywords are what oracle/hdbscan_ref.py assumes
  labels                 oracle.hdbscan_ref = the recorded labels on every tie-decided map and every video's first clustered map
  whole path, oracle     tail_ref.cluster_loop (replayed labels) = the maps after the reference's loop; tail_ref centres;
                         pipeline_ref.crop_from_maps at every recorded stage down to the windows
  product host code      S.blend_flags against the inputs the reference's calls received; pipeline.plan_call in batches of 3 and
                         8; fill, focus stability on the FILTERED maps, series, boxes, time shift
  staleness              three videos and part B regenerated where the reference tree is present

Gates: those of tests/test_refpath_host.py and no other.  Everything is equal except: a centre behind k-means within 1e-12 px, the
product's native series within 1e-9 px (interpolated) and 1e-6 px (smoothed)."""
import os

import numpy as np
import pytest

import refpath_clustered_cases as RCC
from oracle import hdbscan_ref as H, pipeline_ref as P, tail_ref as T
from retargetvid_amd import pipeline, smartVidCrop as S, temporal

CASES, DIRECT = RCC.load()
IDS = [RCC.case_id(c) for c in CASES]
REPLAY = RCC.replay(CASES)
KM_CENTRE_TOL = 1e-12
INTERP_TOL, SMOOTH_TOL = 1e-9, 1e-6
REFERENCE_DIR = os.environ.get('SVC_REFERENCE_DIR', '/root/reference')


def _same_nan(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_census_and_caps():
    assert 20 <= len(CASES) <= 30 and 35 <= len(DIRECT) <= 60
    assert os.path.getsize(RCC.PATH) <= 1000000
    frames = sum(c['fc'] for c in CASES)
    amb = sum(int(c['ambiguous'].sum()) for c in CASES)
    assert amb <= 0.005 * frames
    assert all(not c['ambiguous'].any() for c in CASES if c['CP']['shift_time'])
    assert {c['set'] for c in CASES} == {'default_km', 'default_argmax', 'default_sum', 'best_argmax', 'best_km'}
    sizes = [(c['w_orig'], c['h_orig']) for c in CASES]
    assert set(sizes) == {(640, 360), (360, 640), (720, 720)} and sizes.count((720, 720)) <= 3
    want_best = dict(t_threshold=90, hdbscan_min=5, hdbscan_min_samples=3, select_sum=1, focus_stability=True, min_d_jump=1,
                     lp_cutoff=1, lp_order=2, loess_filt=0)
    for c in CASES:
        CP, n = c['CP'], c['fc_sel']
        assert CP['clust_filt'] is True and CP['op_close'] is False and CP['resize_factor'] == 1.0
        if c['best']:
            assert all(CP[k] == v for k, v in want_best.items())
        assert 40 <= c['fc'] <= 150 and n <= 32
        assert int((c['prep'] >= CP['t_threshold']).reshape(n, -1).sum(1).max()) <= 3000
        assert c['calls_in'].shape == c['calls_out'].shape == c['after'].shape == c['thr'].shape and len(c['labels']) == n
        for i in range(n):
            npts = int((c['calls_in'][i] > 0).sum())
            assert (c['labels'][i] is not None) == (npts > CP['hdbscan_min'] + 1)           # the gate, as the reference took it
            assert c['labels'][i] is None or len(c['labels'][i]) == npts
    # the counts the generator gated the fixture on (RCC.census: the blends are those the reference's calls received, the winner
    # is the cluster the reference left in the map it returned)
    z = RCC.census(CASES)
    print('census:', z)
    assert z['tied'] >= 12 and z['tied3'] >= 4 and z['not_raster_first'] >= 4 and z['not_largest'] >= 4
    assert z['sum_not_label0'] >= 6
    assert z['chains3'] >= 8 and z['chains5'] >= 2 and z['blends_after_loss'] >= 6 and z['wraps'] >= 2 and z['lt_videos'] >= 2
    assert z['chains_without_loss'] == 0          # in every chain the filter removed points from at least one map that is blended on
    assert z['gate_plus1'] >= 1 and z['gate_plus2'] >= 1 and z['noise_zeroed'] >= 1 and z['empty_calls'] >= 3
    fam = {c['family'] for c in CASES}
    assert fam >= {'no_cut', 'cut_at_sel_1', 'cut_at_fc_sel_2', 'cut_at_fc_sel_3', 'cuts_one_apart', 'cuts_two_apart',
                   'empty_chain_start', 'empty_chain_middle', 'empty_chain_end', 'wrap', 'gates'}
    by = {c['family']: c for c in CASES}
    starts = lambda c: [int(s[0]) for s in c['segmentation_sel']]       # noqa: E731
    assert starts(by['no_cut']) == [0] and starts(by['cut_at_sel_1']) == [0, 1]
    assert starts(by['cut_at_fc_sel_2'])[-1] == by['cut_at_fc_sel_2']['fc_sel'] - 2
    assert starts(by['cut_at_fc_sel_3'])[-1] == by['cut_at_fc_sel_3']['fc_sel'] - 3
    assert np.diff(starts(by['cuts_one_apart']))[-1] == 1 and np.diff(starts(by['cuts_two_apart']))[-1] == 2
    for k, d in (('empty_chain_start', -1), ('empty_chain_middle', 0), ('empty_chain_end', 2)):
        assert not by[k]['prep'][starts(by[k])[-1] + d].any()
    # part B
    names = {b['name'] for b in DIRECT}
    assert names >= {'tie%d_winner_%s_ss%d' % (k, p, s) for k in (2, 3, 4) for p in ('first', 'middle', 'last') for s in (0, 1, 2, 3)}
    assert names >= {'label0_loses_max', 'label0_loses_sum', 'all_noise', 'one_cluster_no_noise', 'empty', 'gate_min5_plus1',
                     'gate_min5_plus2', 'gate_min26_plus1', 'gate_min26_plus2', 'sum_past_2_16'}
    for b in DIRECT:
        assert 24 <= b['map'].shape[0] <= 60 and 40 <= b['map'].shape[1] <= 90
        if b['name'].startswith('tie'):
            w = RCC.weights(b['map'], b['labels'], b['CP']['select_sum'])
            assert len({v[0] for v in w}) == 1 and len(w) == int(b['name'][3])          # all tied; with select_sum 1: equal sums
    d = {b['name']: b for b in DIRECT}
    assert np.array_equal(d['all_noise']['out'], d['all_noise']['map']) and d['all_noise']['map'].any()
    big = RCC.weights(d['sum_past_2_16']['map'], d['sum_past_2_16']['labels'], 1)
    assert big[1][0] > 65536 > big[0][0] > big[1][0] % 65536


# ---- the glue of the filter -------------------------------------------------------------------------------------------------------
def test_oracle_filter_with_replayed_labels_equals_every_recorded_call():
    n = 0
    for c in CASES:
        for i in range(c['fc_sel']):
            got = T.clustering_filt(c['calls_in'][i], c['CP'], labels_fn=REPLAY)
            assert np.array_equal(got, c['calls_out'][i]), (RCC.case_id(c), i)
            n += 1
    for b in DIRECT:
        got = T.clustering_filt(b['map'], b['CP'], labels_fn=RCC.replay([b]))      # (labels None: replay has nothing to hand out)
        assert np.array_equal(got, b['out']), b['name']
        n += 1
    assert n == sum(c['fc_sel'] for c in CASES) + len(DIRECT)


def test_constructor_keywords_are_what_the_oracle_assumes():
    for c in CASES:
        k = c['ctor']
        assert k['metric'] == 'sqeuclidean' and k['cluster_selection_method'] == 'eom' and k['allow_single_cluster'] is True
        assert k['min_cluster_size'] == c['CP']['hdbscan_min'] and k['min_samples'] == c['CP']['hdbscan_min_samples']
        assert set(k) == {'min_cluster_size', 'min_samples', 'metric', 'approx_min_span_tree', 'gen_min_span_tree',
                          'cluster_selection_method', 'core_dist_n_jobs', 'allow_single_cluster'}


def test_oracle_hdbscan_equals_the_recorded_labels_on_tie_decided_and_first_maps():
    n_tied = 0
    for c in CASES:
        first = next(i for i in range(c['fc_sel']) if c['labels'][i] is not None)
        picks = {first} | {i for i in range(c['fc_sel']) if len(RCC.tied(c, i)) >= 2}
        n_tied += len(picks) - 1
        for i in sorted(picks):
            X = np.argwhere(c['calls_in'][i] > 0).astype(np.int64)
            got = H.hdbscan_labels(X, c['CP']['hdbscan_min'], c['CP']['hdbscan_min_samples'])
            assert np.array_equal(got, c['labels'][i]), (RCC.case_id(c), i)
    assert n_tied >= 12


# ---- the whole path, oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_oracle_equals_the_reference_at_every_stage(c):
    CP = dict(c['CP'])
    n = c['fc_sel']
    # the loop alone, from the thresholded maps
    hwn = np.ascontiguousarray(np.transpose(c['thr'], (1, 2, 0))).copy()
    T.cluster_loop(hwn, T.segm_cuts_of(c['segmentation_sel']), CP, labels_fn=REPLAY)
    assert np.array_equal(np.transpose(hwn, (2, 0, 1)), c['after'])
    assert np.array_equal(c['after'], c['calls_out'])
    dx, dy = T.centers(hwn, CP)
    raw = np.stack([np.array([np.nan if v is None else v for v in col], np.float64) for col in (dx, dy)], 1)
    exact = not CP['com_km']
    close = (lambda a, b, tol: _same_nan(a, b)) if exact else (
        lambda a, b, tol: np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(np.asarray(a, np.float64) - b), initial=0.0) <= tol)
    assert close(raw, c['centres_raw'], KM_CENTRE_TOL)
    # the whole path from the maps the reference held
    seg, seg_sel = c['segmentation'], c['segmentation_sel']
    VD = dict(smaps=np.ascontiguousarray(np.transpose(c['raw'], (1, 2, 0))), segmentation=seg, segmentation_sel=seg_sel,
              true_inds=c['true_inds'].tolist(), inds_to_orig=c['inds_to_orig'].tolist(), fr=c['fr'], fc=c['fc'], fc_sel=n,
              h_orig=c['h_orig'], w_orig=c['w_orig'], h_process=c['h_process'], w_process=c['w_process'])
    st = {}
    VD = P.crop_from_maps(VD, CP, stage=st, labels_fn=REPLAY)
    assert np.array_equal(np.transpose(st['thresholded'], (2, 0, 1)), c['thr'])
    assert np.array_equal(np.transpose(st['filtered'], (2, 0, 1)), c['after'])
    pair = lambda t: np.stack([np.asarray(t[0], np.float64), np.asarray(t[1], np.float64)], 1)      # noqa: E731
    assert close(pair(st['centres_filled']), c['centres_filled'], KM_CENTRE_TOL) and np.array_equal(c['centres_filled'], c['dxnf'])
    assert close(pair(st['centres_stab']), c['centres_stab'], KM_CENTRE_TOL)
    assert [float(v) for v in st['jumps']] == c['jumps'].tolist() and st['jumps_inds'] == c['jumps_inds']
    assert close(pair((VD['dxi'], VD['dyi'])), c['dxi'], INTERP_TOL)
    assert close(pair((VD['dxs'], VD['dys'])), c['dxs'], SMOOTH_TOL)
    assert (VD['w_final'], VD['h_final'], VD['fbb_w'], VD['fbb_h']) == (c['w_final'], c['h_final'], c['fbb_w'], c['fbb_h'])
    ok = ~c['ambiguous']
    assert int(ok.sum()) == c['fc'] - int(c['ambiguous'].sum())
    assert np.array_equal(np.asarray(st['bbs_pre'])[ok], c['bbs_pre'][ok])
    assert np.array_equal(np.asarray(VD['bbs'])[ok], c['bbs'][ok])


# ---- the product's host code ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_blend_flags_are_the_blends_the_references_calls_received(c):
    n = c['fc_sel']
    flags = S.blend_flags(n, c['segmentation_sel'])
    seen = RCC.flags_seen(c)
    assert len(flags) == n and not flags[n - 1]
    for i in range(n - 1):
        if seen[i]:                          # the reference's call i + 1 received something else than the thresholded map i + 1
            assert flags[i], i
        if flags[i]:                         # ... and what it received is the blend of ITS returned map i into the thresholded map i + 1
            assert np.array_equal(c['calls_in'][i + 1], T.blend_next(c['calls_out'][i], c['thr'][i + 1])), i
        else:
            assert np.array_equal(c['calls_in'][i + 1], c['thr'][i + 1]), i
    assert np.array_equal(c['calls_in'][0], c['thr'][0])


def test_blend_flags_stop_before_fc_sel_2_where_the_rule_would_set_one():
    """The `<` of i < fc_sel - 2: the cut list holds the last scene's end (fc_sel - 1), so the rule's three-frame test is true at
    fc_sel - 2 in every video; the reference's call fc_sel - 1 received its thresholded map all the same."""
    n_lt = 0
    for c in CASES:
        n = c['fc_sel']
        flags = S.blend_flags(n, c['segmentation_sel'])
        assert int(c['segmentation_sel'][-1][1]) == n - 1 and not flags[n - 2]
        assert np.array_equal(c['calls_in'][n - 1], c['thr'][n - 1])
        n_lt += bool(flags[n - 3])
    assert n_lt >= 2


@pytest.mark.parametrize('batch', [3, 8])
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_plan_call_in_batches_processes_every_map_once_behind_its_final_predecessor(c, batch):
    """pipeline.plan_call driven as StreamPipeline drives it (the span kept whole), the flags it hands the device acted out with
    the oracle's filter and blend: every map is filtered exactly once, a blended map only after its predecessor is final, and
    the maps are those after the reference's loop."""
    n = c['fc_sel']
    bnext = [bool(v) for v in S.blend_flags(n, c['segmentation_sel'])]
    cur = c['thr'].copy()
    times = np.zeros(n, int)
    states, fed = [], 0

    def call(flush):
        flags, done = pipeline.plan_call(states, bnext[:len(states)], flush)
        for i in range(len(states)):
            if i in done:
                assert states[i] == pipeline.RAW
                assert i == 0 or not bnext[i - 1] or blended[i], i           # behind its predecessor: the blend has reached it
                cur[i] = T.clustering_filt(cur[i], c['CP'], labels_fn=REPLAY)
                times[i] += 1
                final[i] = True
            if flags[i] & pipeline.BLEND_NEXT:
                assert final[i] and i + 1 in done and not blended[i + 1]
                cur[i + 1] = T.blend_next(cur[i], cur[i + 1])
                blended[i + 1] = True
        for i in done:
            states[i] = pipeline.FINAL
    final, blended = np.zeros(n, bool), np.zeros(n, bool)
    while fed < n:
        k = min(batch, n - fed)
        states += [pipeline.RAW] * k
        fed += k
        call(False)
    if any(s == pipeline.RAW for s in states):
        call(True)
    assert (times == 1).all() and np.array_equal(cur, c['after'])
    assert np.array_equal(blended[1:], np.asarray(bnext[:-1]))


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_product_host_stages_equal_the_reference_on_filtered_maps(c):
    CP = S.sc_init_crop_params(use_best_settings=c['best'])
    CP.update(c['overrides'])
    assert CP == c['CP']
    xy, still = temporal.fill_empty_centres(c['centres_raw'], c['segmentation_sel'])
    assert still == 0 and np.array_equal(xy, c['centres_filled'])
    if CP['focus_stability']:
        xy, jumps, inds = temporal.focus_stability_native(c['centres_filled'], c['after'], c['fr'], CP)
        assert np.array_equal(xy, c['centres_stab'])
        assert [float(v) for v in jumps] == c['jumps'].tolist() and inds == c['jumps_inds']
    else:
        assert np.array_equal(c['centres_stab'], c['centres_filled']) and c['jumps_inds'] == [] and (c['jumps'] == 255).all()
    xi, yi, xs, ys = temporal.centres_to_series(c['centres_stab'], c['true_inds'], c['segmentation'], c['segmentation_sel'], c['fc'],
                                                c['fr'], CP)
    di = max(np.abs(xi - c['dxi'][:, 0]).max(), np.abs(yi - c['dxi'][:, 1]).max())
    ds = max(np.abs(xs - c['dxs'][:, 0]).max(), np.abs(ys - c['dxs'][:, 1]).max())
    print('%s: interpolated %.3g px, smoothed %.3g px from the reference' % (RCC.case_id(c), di, ds))
    assert di < INTERP_TOL and ds < SMOOTH_TOL
    for sx, sy, ok in ((c['dxs'][:, 0], c['dxs'][:, 1], np.ones(c['fc'], bool)), (xs, ys, ~c['ambiguous'])):
        VD = dict(w_orig=c['w_orig'], h_orig=c['h_orig'], w_process=c['w_process'], h_process=c['h_process'], fc=c['fc'],
                  dxs=sx.tolist(), dys=sy.tolist())
        VD = S.sc_calc_dest_size(VD, CP)
        assert (VD['w_final'], VD['h_final']) == (c['w_final'], c['h_final'])
        VD = S.sc_border_detection(CP, VD)
        VD = S.sc_compute_bb(VD, CP)
        assert (VD['fbb_w'], VD['fbb_h']) == (c['fbb_w'], c['fbb_h'])
        assert np.array_equal(np.asarray(VD['bbs'])[ok], c['bbs_pre'][ok])
        assert np.array_equal(VD['bbs_np'][ok], c['bbs_pre'][ok]) and int(ok.sum()) >= c['fc'] - int(c['ambiguous'].sum())
    assert temporal.shift_time(c['bbs_pre'].tolist(), CP['shift_time']) == c['bbs'].tolist()


def test_focus_stability_saw_jumps_on_either_side_of_its_threshold():
    best = [c for c in CASES if c['best']]
    stats = np.concatenate([c['jumps'] for c in best])
    assert (stats < 60).sum() >= 10 and ((stats >= 60) & (stats < 255)).sum() >= 10
    assert sum(1 for c in best if (c['centres_stab'] != c['centres_filled']).any()) >= 3
    assert {c['set'] for c in best if (c['centres_stab'] != c['centres_filled']).any()} == {'best_argmax', 'best_km'}


# ---- staleness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE_DIR, 'smartVidCrop.py')), reason='the reference tree is not on this machine')
def test_three_videos_and_the_direct_calls_regenerated_from_the_reference_equal_the_fixture():
    """tools/make_golden_refpath_clustered.py run again on three videos (a sum-rule one, the wrap one with focus stability behind
    k-means, an arg-max one with an empty map at a chain's start) and on part B, in a child process so that the stub modules it installs stay out of this one."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import numpy as np, make_golden_refpath_clustered as G, refpath_clustered_cases as RCC\n'
            'ref, stubs = G.setup(%r)\n'
            'want, want_b = RCC.load()\n'
            'def same(v, g):\n'
            '    if isinstance(v, np.ndarray):\n'
            '        return np.array_equal(v, g, equal_nan=v.dtype.kind == "f")\n'
            '    if isinstance(v, list) and any(isinstance(x, np.ndarray) or x is None for x in v):\n'
            '        return len(v) == len(g) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(v, g))\n'
            '    return v == g\n'
            'brecs = G.run_part_b(ref)\n'
            'for i in (2, 9, 18):\n'
            '    out = G.pack([G.generate_case(ref, stubs, i)], brecs)\n'
            '    out["crop_params"] = G.G.crop_params_of(ref)\n'
            '    got, got_b = RCC.split(out)\n'
            '    for k, v in want[i].items():\n'
            '        assert k == "index" or same(v, got[0][k]), (i, k)\n'
            'assert len(got_b) == len(want_b)\n'
            'for a, b in zip(want_b, got_b):\n'
            '    assert all(same(v, b[k]) for k, v in a.items()), a["name"]\n'
            'assert not G.ProxyHDBSCAN.findings\n'
            'print("same")\n') % (os.path.join(root, 'tools'), os.path.join(root, 'tests'), REFERENCE_DIR)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=root, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('same'), out.stderr[-3000:]
