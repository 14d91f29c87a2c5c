"""tests/golden/refpath_clustered_golden.npz read back, as tools/make_golden_refpath_clustered.py recorded it.  Shared by
tests/test_refpath_clustered_host.py and tests/test_gpu_refpath_clustered.py; reads the fixture only.

Part A, one dict per video: the reference's own smart_vid_crop with clust_filt = True, op_close = False, resize_factor = 1.
Everything tests/refpath_cases.py lists (centres_raw .. bbs are now what the reference computed ON THE FILTERED MAPS), and

  CP                   the reference's parameter dict of the video (its defaults or best settings, with `overrides` on top)
  calls_in [n, h, w]   the map every call of sc_clustering_filt received (call i = selected frame i): thr[i], or its blend
  calls_out [n, h, w]  the map it returned
  after [n, h, w]      the maps after the clustering loop
  labels               per call: None where the reference did not call fit_predict, else the labels it was handed for X =
                       np.argwhere(calls_in[i] > 0).  They are scikit-learn's HDBSCAN labels (the project's proxy for the hdbscan
                       package, which is not the reference's code), not the reference's.
  ctor                 the keywords the reference constructed its clusterer with

Part B, `direct`: one dict per direct call of the reference's sc_clustering_filt with a hand-made label vector:
name, CP, map, out, labels (None: fit_predict must not be called)."""
import functools
import json
import os

import numpy as np

import refpath_cases as RC

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'refpath_clustered_golden.npz')
FIX = dict(op_close=False, resize_factor=1.0)


def _cp(crop_params, best, over):
    cp = dict(crop_params[1 if best else 0])
    cp.update(over)
    return cp


def split(z):
    """npz mapping (or the generator's packed dict) -> (videos, direct calls)."""
    cases = RC.split(z)
    crop_params = [json.loads(str(s)) for s in z['crop_params']]
    offs = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)    # noqa: E731
    px = np.array([c['h_process'] * c['w_process'] for c in cases], np.int64)
    n_sel = np.array([c['fc_sel'] for c in cases], np.int64)
    o_map, o_call = offs(n_sel * px), offs(n_sel)
    n_in = np.asarray(z['n_filt_in'], np.int64)
    o_in, o_inmap = offs(n_in), offs(n_in * px)
    nfit = np.asarray(z['nfit'], np.int64)
    o_lab = offs(np.maximum(nfit, 0))
    all_labels = np.asarray(z['labels'])
    for i, c in enumerate(cases):
        c['best'] = c['set'].startswith('best')
        c['CP'] = _cp(crop_params, c['best'], c['overrides'])
        shape = (c['fc_sel'], c['h_process'], c['w_process'])
        c['calls_out'] = np.asarray(z['filt_out'][o_map[i]:o_map[i + 1]]).reshape(shape)
        c['after'] = np.asarray(z['after'][o_map[i]:o_map[i + 1]]).reshape(shape)
        c['calls_in'] = c['thr'].copy()
        idx = np.asarray(z['filt_in_idx'][o_in[i]:o_in[i + 1]], np.int64)
        c['calls_in'][idx] = np.asarray(z['filt_in_maps'][o_inmap[i]:o_inmap[i + 1]]).reshape((-1,) + shape[1:])
        c['labels'] = []
        for j in range(o_call[i], o_call[i + 1]):
            c['labels'].append(None if nfit[j] < 0 else all_labels[o_lab[j]:o_lab[j + 1]].astype(np.int64))
        c['ctor'] = json.loads(str(z['ctor'][i]))
    direct = []
    b_shape = np.asarray(z['b_shape'], np.int64)
    b_nfit = np.asarray(z['b_nfit'], np.int64)
    o_b, o_bl = offs(b_shape[:, 0] * b_shape[:, 1]), offs(np.maximum(b_nfit, 0))
    for j in range(len(b_shape)):
        over = json.loads(str(z['b_over'][j]))
        direct.append(dict(name=str(z['b_name'][j]), CP=_cp(crop_params, False, dict(FIX, **over)),
                           map=np.asarray(z['b_map'][o_b[j]:o_b[j + 1]]).reshape(b_shape[j]),
                           out=np.asarray(z['b_out'][o_b[j]:o_b[j + 1]]).reshape(b_shape[j]),
                           labels=None if b_nfit[j] < 0 else np.asarray(z['b_labels'][o_bl[j]:o_bl[j + 1]]).astype(np.int64)))
    return cases, direct


@functools.lru_cache(maxsize=1)
def load():
    """-> (videos, direct calls)."""
    with np.load(PATH) as z:
        return split(z)


def case_id(c):
    return '%02d_%s_%s' % (c['index'], c['set'], c['family'])


def replay(cases):
    """labels_fn for oracle.tail_ref.clustering_filt: the recorded labels of the point set it is asked about (KeyError for a
    point set the reference never clustered).  cases: videos (labels depend on the point set and the two sizes only), or ONE
    direct call (hand-made labels belong to their call)."""
    table = {}
    for c in cases:
        items = zip(c['calls_in'], c['labels']) if 'calls_in' in c else [(c['map'], c['labels'])]
        for m, lab in items:
            if lab is not None:
                key = (c['CP']['hdbscan_min'], c['CP']['hdbscan_min_samples'], np.argwhere(m > 0).astype(np.int64).tobytes())
                assert key not in table or np.array_equal(table[key], lab)
                table[key] = lab

    def labels_fn(X, mcs, ms):
        return table[(mcs, ms, np.asarray(X, np.int64).tobytes())].copy()
    return labels_fn


def weights(map_in, labels, select_sum):
    """Per cluster 0 .. n - 1: (weight, size, index of its first point in raster order) -- to find which clusters tie; what the
    filter chose is in calls_out (kept)."""
    W = map_in[map_in > 0].astype(np.int64)
    n = len(set(labels.tolist())) - (1 if -1 in labels else 0)
    out = []
    for k in range(n):
        idx = np.flatnonzero(labels == k)
        out.append((int(W[idx].sum()) if select_sum == 1 else int(W[idx].max()), len(idx), int(idx[0])))
    return out


def tied(c, i):
    """Clusters of call i of video c that attain the winning weight ([] where nothing was clustered)."""
    if c['labels'][i] is None:
        return []
    w = weights(c['calls_in'][i], c['labels'][i], c['CP']['select_sum'])
    return [k for k, v in enumerate(w) if v[0] == max(x[0] for x in w)]


def flags_seen(c):
    """Flag i: the reference's input to call i + 1 is not the thresholded map i + 1."""
    n = c['fc_sel']
    return np.array([bool((c['calls_in'][i + 1] != c['thr'][i + 1]).any()) for i in range(n - 1)] + [False])


def kept(map_in, map_out, labels):
    """The cluster the reference's filter KEPT, read from the map it returned: the one label whose points it left non-zero
    (every cluster has non-zero points on the way in).  None where it left no cluster or more than one (a map returned untouched)."""
    left = map_out[map_in > 0] > 0
    ks = sorted(set(labels[left].tolist()) - {-1})
    return ks[0] if len(ks) == 1 and not left[labels != ks[0]].any() else None


def chains(flags):
    """Runs of consecutive flags f .. g -> [(f, g + 1)]: the chain of maps f .. g + 1."""
    out, i, n = [], 0, len(flags)
    while i < n:
        if flags[i]:
            j = i
            while j + 1 < n and flags[j + 1]:
                j += 1
            out.append((i, j + 1))
            i = j + 1
        i += 1
    return out


def census(cases):
    """The counts that tools/make_golden_refpath_clustered.py gates the fixture on and tests/test_refpath_clustered_host.py asserts
    again -- this one copy.  cases: the reader's videos, or the generator's records under the same keys (CP, fc, fc_sel, thr,
    calls_in, calls_out, labels).  Nothing here applies the rules under test: the blends are those the reference's calls
    received (flags_seen), the winner is the cluster the reference left in the map it returned (kept); only which clusters TIE is
    computed, from the map's values and the labels."""
    z = dict(videos=len(cases), frames=0, selected=0, clustered=0, unclustered_nonempty=0, empty_calls=0, lost_points=0, no_cluster=0,
             tied=0, tied3=0, not_raster_first=0, not_largest=0, sum_3plus=0, sum_not_label0=0, equal_sums=0, chains3=0, chains5=0,
             blends=0, blends_after_loss=0, wraps=0, lt_videos=0, gate_plus1=0, gate_plus2=0, max_points=0, noise_zeroed=0,
             chains_without_loss=0)
    for c in cases:
        CP, n = c['CP'], c['fc_sel']
        z['frames'] += c['fc']
        z['selected'] += n
        flags = flags_seen(c)
        z['lt_videos'] += bool(n >= 4 and flags[n - 3] and not flags[n - 2])
        for f, g in chains(flags):
            z['chains3'] += g - f + 1 >= 3
            z['chains5'] += g - f + 1 >= 5
            z['chains_without_loss'] += not any((c['calls_out'][i] != c['calls_in'][i]).any() for i in range(f, g))
        for i in range(n):
            m_in, m_out, lab = c['calls_in'][i], c['calls_out'][i], c['labels'][i]
            npts = int((m_in > 0).sum())
            z['max_points'] = max(z['max_points'], npts)
            if flags[i]:
                z['blends'] += 1
                z['blends_after_loss'] += bool((m_out != m_in).any())
                z['wraps'] += bool((m_out.astype(np.int64) + c['thr'][i + 1].astype(np.int64) >= 256).any())
            z['gate_plus1'] += npts == CP['hdbscan_min'] + 1
            z['gate_plus2'] += npts == CP['hdbscan_min'] + 2
            if lab is None:
                z['empty_calls' if npts == 0 else 'unclustered_nonempty'] += 1
                continue
            z['clustered'] += 1
            z['lost_points'] += bool((m_in != m_out).any())
            z['noise_zeroed'] += bool((lab == -1).any())
            w = weights(m_in, lab, CP['select_sum'])
            win = kept(m_in, m_out, lab)
            if not w or win is None:
                z['no_cluster'] += 1
                continue
            t = [k for k, v in enumerate(w) if v[0] == max(x[0] for x in w)]
            if CP['select_sum'] != 1:
                if len(t) >= 2:
                    z['tied'] += 1
                    z['tied3'] += len(t) >= 3
                    z['not_raster_first'] += w[win][2] != min(w[k][2] for k in t)
                    z['not_largest'] += w[win][1] < max(w[k][1] for k in t)
            else:
                z['equal_sums'] += len(t) >= 2
                z['sum_3plus'] += len(w) >= 3
                z['sum_not_label0'] += len(w) >= 3 and win != 0
    return {k: int(v) for k, v in z.items()}
