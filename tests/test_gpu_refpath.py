"""-m gpu: the product's device path for clust_filt = False (after_ingest: k_threshold, the no-filter centre kernels, the native
host stages) against the reference's OWN smart_vid_crop, as tests/golden/refpath_golden.npz recorded it
(tools/make_golden_refpath.py, tests/refpath_cases.py; the host stages alone and the oracle: tests/test_refpath_host.py).  Reads
only the fixture.  Per video the maps the reference held before sc_threshold are uploaded, the VD dictionary is built from the
recorded bookkeeping and after_ingest runs once:

  maps after engine.threshold_           the reference's thresholded maps, byte for byte (also on a clone from a separate call)
  centres from engine.cluster_center_    NaN where the reference had None; com_km = False: the reference's integers; com_km =
                                         True: the reference's KMeans centre within 1e-12 px, the bound tests/test_oracle_tail.py
                                         keeps between the oracle's mean and KMeans
  fill, focus stability                  dxnf / dynf, the held centres, every jump statistic and jumps_inds: equal (1e-12 px
                                         behind a k-means centre)
  interpolated / smoothed series         1e-9 / 1e-6 px (tests/test_host_native.py)
  w/h_final, fbb_w/h, bbs                equal on every frame the fixture does not mark ambiguous; the count compared is asserted
  ops.iou_boxes                          the reference's doubles on 2 000 pairs, bit for bit"""
import numpy as np
import pytest
import torch

import refpath_cases as RC
from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from retargetvid_amd import ops, smartVidCrop as S

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

CASES, EXTRAS = RC.load()
IDS = [RC.case_id(c) for c in CASES]
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


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_after_ingest_equals_the_reference_from_raw_maps_to_windows(engine, c):
    CP = S.sc_init_crop_params(use_best_settings=c['best'])
    CP.update(c['overrides'])
    exact = not CP['com_km']
    raw = torch.from_numpy(c['raw']).cuda()
    # threshold and centres on a clone, from calls of their own
    clone = raw.clone()
    engine.threshold_(clone, CP['t_threshold'])
    assert np.array_equal(clone.cpu().numpy(), c['thr'])
    xy = engine.cluster_center_(clone, None, CP).cpu().numpy()
    assert np.array_equal(clone.cpu().numpy(), c['thr'])                 # without the cluster filter the maps stay as they are
    assert _centres_match(xy, c['centres_raw'], exact), np.abs(xy - c['centres_raw']).max()
    # the one run
    VD, res = S.after_ingest(_vd(c, raw), CP, engine)
    assert res['result'] == 'smart cropped'
    assert np.array_equal(VD['smaps_dev'].cpu().numpy(), c['thr'])
    assert _centres_match(np.stack([VD['dxnf'], VD['dynf']], 1), c['centres_filled'], exact)
    assert _centres_match(np.stack([VD['dx'], VD['dy']], 1), c['centres_stab'], exact)
    assert VD['jumps_inds'] == c['jumps_inds']
    assert [float(v) for v in VD['jumps']] == c['jumps'].tolist()
    di = np.abs(np.stack([VD['dxi'], VD['dyi']], 1) - c['dxi']).max()
    ds = np.abs(np.stack([VD['dxs_smooth'], VD['dys_smooth']], 1) - c['dxs']).max()
    print('%s: interpolated %.3g px, smoothed %.3g px from the reference' % (RC.case_id(c), di, ds))
    assert di < INTERP_TOL and ds < SMOOTH_TOL
    assert (VD['w_final'], VD['h_final'], VD['fbb_w'], VD['fbb_h']) == (c['w_final'], c['h_final'], c['fbb_w'], c['fbb_h'])
    ok = ~c['ambiguous']
    assert int(ok.sum()) == c['fc'] - int(c['ambiguous'].sum())          # nothing is skipped but what the fixture marks
    got = np.asarray(VD['bbs'], np.int64)
    assert got.shape == (c['fc'], 4)
    if not CP['shift_time'] or ok.all():
        assert np.array_equal(got[ok], c['bbs'][ok])
    assert np.array_equal(VD['bbs_np'], got)
    if not CP['shift_time']:
        assert np.array_equal(got[ok], c['bbs_pre'][ok])


def test_the_fixture_leaves_no_frame_unchecked_beyond_its_cap():
    frames = sum(c['fc'] for c in CASES)
    marked = sum(int(c['ambiguous'].sum()) for c in CASES)
    assert marked <= 0.005 * frames
    assert all(not c['ambiguous'].any() for c in CASES if c['overrides'].get('shift_time'))     # (shifted windows are compared whole)


def test_iou_boxes_equals_the_references_doubles_bit_for_bit():
    a, b, want = EXTRAS['iou_a'], EXTRAS['iou_b'], EXTRAS['iou']
    assert len(want) == 2000
    got = ops.iou_boxes(a, b)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
