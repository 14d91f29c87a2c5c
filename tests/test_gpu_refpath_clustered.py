"""-m gpu: the product's device path for clust_filt = True (after_ingest: k_threshold, the cluster filter with its blend rounds, the
centre kernels, the native host stages) against the reference's OWN smart_vid_crop and sc_clustering_filt, as
tests/golden/refpath_clustered_golden.npz recorded them (tools/make_golden_refpath_clustered.py,
tests/refpath_clustered_cases.py; the oracle and the host code alone: tests/test_refpath_clustered_host.py).  Reads only the
fixture.  The labels in it are scikit-learn's, handed to the reference in the place of the hdbscan package's; the device computes
its own and must arrive at the same maps.

  per video, one after_ingest      maps after the loop byte for byte; centres (NaN where the reference had None; com_km = False:
                                   equal; k-means: 1e-12 px); fill, hold, every jump statistic and jumps_inds; series within
                                   1e-9 / 1e-6 px; sizes; windows on every frame not marked ambiguous (the count is asserted)
  per clustered map                engine.cluster_state: the point list is X, the labels are the recorded ones up to renaming and
                                   exactly on noise, the kept cluster (HDR_KEPT) holds exactly the points the reference left
  every tie-decided map again      through ops.tail_engine(reference=True): the serial hierarchy and hdb::cluster_before
  the streamed form                StreamPipeline.submit_maps in batches of 8 and of 3: the same final maps and centres"""
import numpy as np
import pytest
import torch

import refpath_clustered_cases as RCC
from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from retargetvid_amd import ops, pipeline as PL, smartVidCrop as S

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

CASES, DIRECT = RCC.load()
IDS = [RCC.case_id(c) for c in CASES]
KM_CENTRE_TOL = 1e-12
INTERP_TOL, SMOOTH_TOL = 1e-9, 1e-6


def _vd(c, maps):
    """What the ingest hands on (smartVidCrop._ingest_dict), from the reference's bookkeeping."""
    return dict(smaps_dev=maps, segmentation=c['segmentation'].copy(), segmentation_sel=c['segmentation_sel'].copy(),
                true_inds=c['true_inds'].tolist(), inds_to_orig=c['inds_to_orig'].tolist(), fr=c['fr'], fc=c['fc'], fc_sel=c['fc_sel'],
                h_orig=c['h_orig'], w_orig=c['w_orig'], h_process=c['h_process'], w_process=c['w_process'],
                n_net_maps=int(c['raw'].reshape(c['fc_sel'], -1).any(1).sum()))


def _centres_match(got, want, exact):
    got, want = np.asarray(got, np.float64).reshape(-1, 2), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if exact:
        return np.array_equal(got, want, equal_nan=True)
    return float(np.nanmax(np.abs(got - want), initial=0.0)) <= KM_CENTRE_TOL


def _state_is_the_references(eng, i, c, k=None):
    """Map i of the engine's last call is call k (default i) of video c: point list, labels, kept cluster."""
    k = i if k is None else k
    m_in, m_out, want = c['calls_in'][k], c['calls_out'][k], c['labels'][k]
    st = eng.cluster_state(i, m_in.size)
    X = np.stack([st['pts'] & 255, (st['pts'] >> 8) & 255], 1).astype(np.int64)
    assert np.array_equal(X, np.argwhere(m_in > 0)), k
    hdr = st['hdr']
    assert hdr[ops.HDR_N] == len(X) and bool(hdr[ops.HDR_CLUSTERED]) == (want is not None), k
    if want is None:
        assert np.array_equal(m_out, m_in)
        return
    got = st['labels']
    assert np.array_equal(want < 0, got < 0), k
    pairs = {(a, b) for a, b in zip(want[want >= 0], got[got >= 0])}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}), 'labels of map %d' % k
    assert hdr[ops.HDR_NSEL] == len({a for a, _ in pairs})                # clusters selected = the reference's n_clusters
    kept = X[got == hdr[ops.HDR_KEPT]] if hdr[ops.HDR_KEPT] >= 0 else X
    assert np.array_equal(kept, np.argwhere(m_out > 0)), 'kept cluster of map %d' % k


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_after_ingest_equals_the_reference_from_raw_maps_to_windows(engine, c):
    CP = S.sc_init_crop_params(use_best_settings=c['best'])
    CP.update(c['overrides'])
    assert CP == c['CP'] and CP['clust_filt']
    exact = not CP['com_km']
    n = c['fc_sel']
    # the filter and the centres on thresholded maps, from a call of their own: the centres before the fill
    thr = torch.from_numpy(c['thr']).cuda()
    xy = engine.cluster_center_(thr, S.blend_flags(n, c['segmentation_sel']), CP).cpu().numpy()
    assert np.array_equal(thr.cpu().numpy(), c['after'])
    assert _centres_match(xy, c['centres_raw'], exact), np.nanmax(np.abs(xy - c['centres_raw']))
    # the one run, from the maps the reference held before sc_threshold
    VD, res = S.after_ingest(_vd(c, torch.from_numpy(c['raw']).cuda()), CP, engine)
    assert res['result'] == 'smart cropped'
    assert np.array_equal(VD['smaps_dev'].cpu().numpy(), c['after'])
    for i in range(n):                                                    # (the state of that run's call)
        _state_is_the_references(engine, i, c)
    assert _centres_match(np.stack([VD['dxnf'], VD['dynf']], 1), c['centres_filled'], exact)
    assert _centres_match(np.stack([VD['dx'], VD['dy']], 1), c['centres_stab'], exact)
    assert VD['jumps_inds'] == c['jumps_inds']
    assert [float(v) for v in VD['jumps']] == c['jumps'].tolist()
    di = np.abs(np.stack([VD['dxi'], VD['dyi']], 1) - c['dxi']).max()
    ds = np.abs(np.stack([VD['dxs_smooth'], VD['dys_smooth']], 1) - c['dxs']).max()
    print('%s: interpolated %.3g px, smoothed %.3g px from the reference' % (RCC.case_id(c), di, ds))
    assert di < INTERP_TOL and ds < SMOOTH_TOL
    assert (VD['w_final'], VD['h_final'], VD['fbb_w'], VD['fbb_h']) == (c['w_final'], c['h_final'], c['fbb_w'], c['fbb_h'])
    ok = ~c['ambiguous']
    assert int(ok.sum()) == c['fc'] - int(c['ambiguous'].sum())          # nothing is skipped but what the fixture marks
    got = np.asarray(VD['bbs'], np.int64)
    assert got.shape == (c['fc'], 4) and not CP['shift_time']
    assert np.array_equal(got[ok], c['bbs'][ok]) and np.array_equal(got[ok], c['bbs_pre'][ok])
    assert np.array_equal(VD['bbs_np'], got)


@pytest.fixture(scope='module')
def serial_engine():
    eng = ops.tail_engine(reference=True)
    yield eng
    eng.close()


def test_every_tie_decided_map_through_the_serial_hierarchy(serial_engine):
    """ops.tail_engine(reference=True): k_tree and its hdb::cluster_before chooser, on every map of part A on which two or more
    clusters attain the winning weight (only there does the numbering of the clusters decide): maps, centres, state."""
    n_maps = 0
    for c in CASES:
        picks = [i for i in range(c['fc_sel']) if len(RCC.tied(c, i)) >= 2]
        if not picks:
            continue
        maps = torch.from_numpy(c['calls_in'][picks]).cuda()
        xy = serial_engine.cluster_center_(maps, None, c['CP']).cpu().numpy()
        assert np.array_equal(maps.cpu().numpy(), c['calls_out'][picks]), RCC.case_id(c)
        assert _centres_match(xy, c['centres_raw'][picks], not c['CP']['com_km']), RCC.case_id(c)
        for j, i in enumerate(picks):
            _state_is_the_references(serial_engine, j, c, i)
        n_maps += len(picks)
    assert n_maps >= 12


@pytest.mark.parametrize('batch', [8, 3])
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_stream_pipeline_gives_the_references_maps_and_centres(engine, c, batch):
    n, h, w = c['thr'].shape
    flags = S.blend_flags(n, c['segmentation_sel'])
    assert flags.any()                                                    # every video has a chain (the first scene's start)
    out = torch.zeros((n, h, w), dtype=torch.uint8, device='cuda')
    pipe = PL.StreamPipeline(engine, c['CP'], h, w, batch=batch, ring_batches=6, max_span_batches=3, maps_out=out)
    dm = torch.from_numpy(c['thr']).cuda()
    got = {}
    for s0 in range(0, n, batch):
        if len(pipe.calls) >= pipe.depth:
            got.update({g: (x, y) for g, x, y in pipe.collect()})
        pipe.submit_maps(dm[s0:s0 + batch], flags[s0:s0 + batch])
    got.update({g: (x, y) for g, x, y in pipe.finish()})
    assert sorted(got) == list(range(n))
    assert np.array_equal(out.cpu().numpy(), c['after'])
    assert _centres_match(np.array([got[i] for i in range(n)], np.float64), c['centres_raw'], not c['CP']['com_km'])
