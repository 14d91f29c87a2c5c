"""tests/golden/refpath_golden.npz read back: one dict per video, as tools/make_golden_refpath.py recorded it from the reference's
own smart_vid_crop (clust_filt = False).  Shared by tests/test_refpath_host.py and tests/test_gpu_refpath.py; reads the fixture
only.  Per video:

  set, family, tags, overrides (the CP keys set on top of the reference's dict), best, fr, fc, fc_sel, w_orig, h_orig, trans_inds
  ingest_pickle:       true_inds, inds_to_orig, segmentation, segmentation_sel, h_process, w_process, raw [n, h, w] (the maps the
                       reference held before sc_threshold), lost_idx / prep (the prepared maps; they differ from raw at lost_idx)
  sc_threshold:        thr [n, h, w]
  centres:             centres_raw [n, 2] (NaN = None) -> centres_filled (dxnf / dynf) -> centres_stab (after the focus hold)
  jumps, jumps_inds
  dxi, dxs [fc, 2]     interpolated; smoothed, as sc_compute_bb receives them
  w_final, h_final, fbb_w, fbb_h, bbs_pre, bbs [fc, 4] (before / after sc_shift_time), ambiguous [fc]"""
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'refpath_golden.npz')
PER_SEL = ('true_inds', 'centres_raw', 'centres_filled', 'jumps', 'dxnf', 'centres_stab')
PER_FRAME = ('inds_to_orig', 'dxi', 'dxs', 'bbs_pre', 'bbs', 'ambiguous')
PER_SCENE = ('segmentation', 'segmentation_sel')


def split(z):
    """npz mapping (or the generator's packed dict) -> list of per-video dicts."""
    names = [str(v) for v in z['meta_names']]
    meta = np.asarray(z['meta'])
    col = lambda k: meta[:, names.index(k)].astype(np.int64)          # noqa: E731
    offs = lambda counts: np.concatenate([[0], np.cumsum(counts)])    # noqa: E731
    o_sel, o_frame, o_scene = offs(col('fc_sel')), offs(col('fc')), offs(col('n_scenes'))
    o_jump, o_trans, o_lost = offs(col('n_jumps_inds')), offs(col('n_trans')), offs(col('n_lost'))
    px = col('h_process') * col('w_process')
    o_map, o_lmap = offs(col('fc_sel') * px), offs(col('n_lost') * px)
    cases = []
    for i in range(len(meta)):
        c = {k: int(meta[i, j]) for j, k in enumerate(names)}
        c['index'] = i
        for k in ('set', 'family'):
            c[k] = str(z[k][i])
        c['tags'] = [t for t in str(z['tags'][i]).split(',') if t]
        c['overrides'] = json.loads(str(z['overrides'][i]))
        c['best'] = c['set'] == 'best'
        c['fr'] = int(z['fr'][i]) if bool(z['fr_is_int'][i]) else float(z['fr'][i])
        for keys, o in ((PER_SEL, o_sel), (PER_FRAME, o_frame), (PER_SCENE, o_scene)):
            for k in keys:
                c[k] = np.asarray(z[k][o[i]:o[i + 1]])
        c['trans_inds'] = [int(v) for v in z['trans_inds'][o_trans[i]:o_trans[i + 1]]]
        c['jumps_inds'] = [int(v) for v in z['jumps_inds'][o_jump[i]:o_jump[i + 1]]]
        c['lost_idx'] = np.asarray(z['lost_idx'][o_lost[i]:o_lost[i + 1]])
        shape = (c['fc_sel'], c['h_process'], c['w_process'])
        c['raw'] = np.asarray(z['raw'][o_map[i]:o_map[i + 1]]).reshape(shape)
        c['thr'] = np.asarray(z['thr'][o_map[i]:o_map[i + 1]]).reshape(shape)
        c['prep'] = c['raw'].copy()
        c['prep'][c['lost_idx']] = np.asarray(z['lost_maps'][o_lmap[i]:o_lmap[i + 1]]).reshape((-1,) + shape[1:])
        cases.append(c)
    return cases


@functools.lru_cache(maxsize=1)
def load():
    """-> (cases, extras): extras = dict(iou_a, iou_b, iou, crop_params [default dict, best dict])."""
    with np.load(PATH) as z:
        cases = split(z)
        extras = dict(iou_a=z['iou_a'], iou_b=z['iou_b'], iou=z['iou'], crop_params=[json.loads(str(s)) for s in z['crop_params']])
    return cases, extras


def case_id(c):
    return '%02d_%s_%s' % (c['index'], c['set'], c['family'])
