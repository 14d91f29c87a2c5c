"""-m gpu: border detection on the device (sc_border_detection, smartVidCrop.py:842-924).  The profile kernels against numpy on
host copies (exact), the fused form against the unfused one, and letterboxed / pillarboxed videos through smart_vid_crop, its
streaming ingest, its feature cache, the multi-video scheduler and the renderer.  Host arithmetic and the reference's own
numbers: tests/test_border_host.py."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import tail_ref as T
from retargetvid_amd import ops, render, scheduler, smartVidCrop as S, synth
from test_oracle_unisal import ELEVEN

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

KEYS = ('border_t', 'border_b', 'border_l', 'border_r')
SHAPES = sorted(set(ELEVEN.values())) + [(35, 35), (141, 249)]


def _np_profile(maps):
    """[n, h, w] u8 on the host -> [n, h + w]: row maxima, then column maxima."""
    return np.concatenate([maps.max(2), maps.max(1)], 1).astype(np.int32)


def _np_borders(f_col, f_row, tb, h, w, ho, wo):
    """Steps 2-4 of the reference restated with its loops (smartVidCrop.py:880-913) -> (t, b, l, r) in original pixels."""
    def count(f):
        k = 0
        for v in f:
            if int(v) > tb:
                break
            k += 1
        return k
    t, b, l, r = count(f_col), count(f_col[::-1]), count(f_row), count(f_row[::-1])
    t, b, l, r = min(t, int(h * 0.45)), min(b, int(h * 0.45)), min(l, int(w * 0.45)), min(r, int(w * 0.45))
    return int((ho / h) * t), int((ho / h) * b), int((wo / w) * l), int((wo / w) * r)


def _crafted(n, h, w, seed):
    """n raw maps: all zero, all 255, one pixel in each corner, bars, noise, in turn."""
    rng = np.random.RandomState(seed)
    m = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        k = i % 9
        if k == 1:
            m[i] = 255
        elif 2 <= k <= 5:
            m[i, (0, 0, h - 1, h - 1)[k - 2], (0, w - 1, 0, w - 1)[k - 2]] = rng.randint(1, 256)
        elif k == 6:                                     # bars: dark rows above and below, dark columns left and right
            m[i] = rng.randint(0, 256, (h, w))
            m[i, :rng.randint(1, h // 3)] = rng.randint(0, 8)
            m[i, h - rng.randint(1, h // 3):] = rng.randint(0, 8)
            m[i, :, :rng.randint(1, w // 3)] = rng.randint(0, 8)
            m[i, :, w - rng.randint(1, w // 3):] = 0
        elif k == 7:
            m[i] = rng.randint(0, 256, (h, w))
        elif k == 8:                                     # sparse noise: most rows and columns stay dark
            ys, xs = rng.randint(0, h, 5), rng.randint(0, w, 5)
            m[i, ys, xs] = rng.randint(1, 256, 5)
    return m


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_border_profile_equals_numpy_at_every_map_shape(engine, shape):
    h, w = shape
    for n in (0, 1, 33, 300):
        a, b = _crafted(n, h, w, seed=h * w + n), _crafted(n, h, w, seed=h * w + n + 1)[::-1].copy()
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        p = engine.border_profile(da)
        assert p.dtype == torch.int32 and tuple(p.shape) == (n, h + w)
        assert np.array_equal(p.cpu().numpy(), _np_profile(a)), (shape, n)
        q = engine.border_profile(db, out=p)             # max-combined into the rows, not overwritten
        assert q is p
        assert np.array_equal(p.cpu().numpy(), np.maximum(_np_profile(a), _np_profile(b))), (shape, n)
        assert torch.equal(da.cpu(), torch.from_numpy(a))                            # the maps are only read
        if n:
            assert np.array_equal(p.amax(0).cpu().numpy(), np.maximum(_np_profile(a), _np_profile(b)).max(0))


def test_border_profile_counts_under_its_own_profiling_class(engine):
    m = torch.from_numpy(_crafted(33, 140, 250, seed=3)).cuda()
    engine.profile_enable('border')
    try:
        engine.border_profile(m)
        engine.border_profile(m)
        ms, cnt = engine.profile_read()
    finally:
        engine.profile_enable(None)
    assert cnt == 2 and ms >= 0.0


@pytest.mark.parametrize('shape', [(140, 250), (250, 140), (249, 249)], ids=lambda s: '%dx%d' % s)
def test_fused_profile_leaves_maps_and_census_alone_and_equals_the_unfused_profile(engine, shape):
    h, w = shape
    n = 37                                                # more than one chunk of 32
    fr = torch.from_numpy(synth.blob_frames(n, h, w, seed=h + w)).cuda()
    raw = engine.saliency(fr)
    want = _np_profile(raw.cpu().numpy())
    for t in (0, 1, 120, 255):
        c0 = torch.zeros((n, 4), dtype=torch.int32, device='cuda') if t else None
        m0 = engine.saliency(fr, threshold=t, census=c0)
        for with_census in ((True, False) if t else (False,)):
            c1 = torch.zeros((n, 4), dtype=torch.int32, device='cuda') if with_census else None
            p1 = torch.zeros((n, h + w), dtype=torch.int32, device='cuda')
            m1 = engine.saliency(fr, threshold=t, census=c1, profile=p1)
            assert torch.equal(m1, m0), (shape, t)
            if with_census:
                assert torch.equal(c1, c0), (shape, t)
            assert np.array_equal(p1.cpu().numpy(), want), (shape, t)
    # the handle's own census (svc_threshold_census) counts the same with and without the profile
    engine.threshold_census(reset=True)
    engine.saliency(fr, threshold=120)
    a = engine.threshold_census(reset=True)
    engine.saliency(fr, threshold=120, profile=torch.zeros((n, h + w), dtype=torch.int32, device='cuda'))
    b = engine.threshold_census(reset=True)
    assert a == b and a['maps'] == n
    # rows are max-combined
    p = torch.full((n, h + w), 7, dtype=torch.int32, device='cuda')
    engine.saliency(fr, threshold=120, profile=p)
    assert np.array_equal(p.cpu().numpy(), np.maximum(want, 7))


def test_fused_profile_is_identical_under_four_streams_at_once(synthetic_sd):
    """The pattern of test_gpu_parity's reproducibility test: four engines on four streams, the same 32 frames; maps, census and
    profile of every pass equal the single-stream ones (atomic maxima do not depend on the order of arrival)."""
    fr = torch.from_numpy(synth.blob_frames(32, 140, 250, seed=0)).cuda()
    engs = [ops.Engine(synthetic_sd) for _ in range(4)]
    try:
        sts = scheduler.lane_streams(torch.device('cuda', torch.cuda.current_device()), 4)
        ref_c = torch.zeros((32, 4), dtype=torch.int32, device='cuda')
        ref_m = engs[0].saliency(fr, threshold=120, census=ref_c).clone()
        ref_p = engs[0].border_profile(engs[0].saliency(fr))
        torch.cuda.synchronize()
        outs = [torch.empty_like(ref_m) for _ in range(4)]
        cens = [torch.empty_like(ref_c) for _ in range(4)]
        profs = [torch.empty_like(ref_p) for _ in range(4)]
        for it in range(40):
            for i in range(4):
                with torch.cuda.stream(sts[i]):
                    cens[i].zero_()
                    profs[i].zero_()
                    engs[i].saliency(fr, out=outs[i], threshold=120, census=cens[i], profile=profs[i])
            torch.cuda.synchronize()
            for i in range(4):
                assert torch.equal(outs[i], ref_m) and torch.equal(cens[i], ref_c) and torch.equal(profs[i], ref_p), (it, i)
    finally:
        for e in engs:
            e.close()


# ---- whole videos -------------------------------------------------------------------------------------------------------

def _barred_video(n, seed, kind, bar, h=360, w=640, trans=None):
    """synth.blob_frames pasted between black bars: 'letterbox' = bars of `bar` rows above and below, 'pillarbox' = bars of
    `bar` columns left and right, 'full' = no bars."""
    fr = np.zeros((n, h, w, 3), np.uint8)
    if kind == 'letterbox':
        fr[:, bar:h - bar] = synth.blob_frames(n, h - 2 * bar, w, seed=seed)
    elif kind == 'pillarbox':
        fr[:, :, bar:w - bar] = synth.blob_frames(n, h, w - 2 * bar, seed=seed)
    else:
        fr = synth.blob_frames(n, h, w, seed=seed)
    return dict(fr=30.0, frame_count=n, w=w, h=h, frames=fr, trans_inds=list(trans or [0, n]), name='%s_%d_%d' % (kind, seed, n))


def _raw_profile(engine, video, CP):
    """(f_col, f_row, h, w) of the video's RAW maps, taken once with the unfused call and reduced with numpy."""
    raw = S.ingest_frames(video, dict(CP, t_border=-1), engine)['smaps_dev'].cpu().numpy()
    M = raw.max(0)
    return M.max(1), M.max(0), raw.shape[1], raw.shape[2]


K_EDGE = 3                 # t_border = the brightest of the first K_EDGE rows (columns) of the profile: at least K_EDGE of them are blank
# (kind, seed, bar): seeds for which the synthetic checkpoint's maps give 0 < t_border < 255 (asserted, never skipped)
E2E = [('letterbox', 11, 50), ('pillarbox', 12, 90)]


def _t_border_for(kind, f_col, f_row):
    return int((f_col if kind == 'letterbox' else f_row)[:K_EDGE].max())


@pytest.mark.parametrize('kind,seed,bar', E2E, ids=lambda v: str(v))
def test_barred_video_end_to_end_plain_streaming_and_cached(engine, tmp_path, kind, seed, bar):
    CP0 = S.sc_init_crop_params()
    v = _barred_video(100, seed, kind, bar, trans=[0, 41, 100])
    f_col, f_row, h, w = _raw_profile(engine, v, CP0)
    tb = _t_border_for(kind, f_col, f_row)
    print('%s seed %d: t_border %d, f_col[:8] %s f_col[-8:] %s f_row[:8] %s f_row[-8:] %s'
          % (kind, seed, tb, f_col[:8], f_col[-8:], f_row[:8], f_row[-8:]))
    assert 0 < tb < 255
    want = _np_borders(f_col, f_row, tb, h, w, v['h'], v['w'])
    print('borders', want)
    assert want[0 if kind == 'letterbox' else 2] >= int((v['h'] / h if kind == 'letterbox' else v['w'] / w) * K_EDGE) > 0
    for ratio in ('1:3', '3:1'):
        CP = dict(CP0, t_border=tb, out_ratio=ratio)
        VD, res = S.smart_vid_crop(v, CP, save_vid=False, engine=engine)
        assert tuple(VD[k] for k in KEYS) == want
        assert np.array_equal(VD['border_f_col'], f_col) and np.array_equal(VD['border_f_row'], f_row)
        bbs, fw, fh = T.compute_bb(list(VD['dxs_smooth']), list(VD['dys_smooth']), VD['fc'], v['w'], v['h'], w, h,
                                   VD['w_final'], VD['h_final'], borders=want)
        assert (VD['fbb_w'], VD['fbb_h']) == (fw, fh) and VD['bbs'] == [list(b) for b in bbs]
        bb = VD['bbs_np']
        t, b, l, r = want
        assert (bb[:, 0] >= l).all() and (bb[:, 2] <= v['w'] - r).all() and (bb[:, 1] >= t).all() and (bb[:, 3] <= v['h'] - b).all()
        assert ((bb[:, 2] - bb[:, 0]) == fw).all() and ((bb[:, 3] - bb[:, 1]) == fh).all()
        # without border detection the same video gives a larger window on the axis it spans
        VD_off, _ = S.smart_vid_crop(v, dict(CP, t_border=-1), save_vid=False, engine=engine)
        assert tuple(VD_off[k] for k in KEYS) == (0, 0, 0, 0) and VD_off['fbb_w'] * VD_off['fbb_h'] >= fw * fh
        if ratio == ('1:3' if kind == 'letterbox' else '3:1'):         # (the window shrinks on the axis it spans fully, :1005-1010)
            assert VD_off['fbb_w'] * VD_off['fbb_h'] > fw * fh
        # the streaming ingest (the tail runs inside it: the profile is taken before its threshold) and the feature cache
        VD_s, _ = S.smart_vid_crop(v, CP, save_vid=False, engine=engine, stream_batch=32)
        assert 'xy_stream' in VD_s
        cache = os.path.join(str(tmp_path), v['name'] + '.pkl')
        if ratio == '1:3':
            assert not os.path.isfile(cache)
            VD_w, _ = S.smart_vid_crop(v, CP, save_vid=False, engine=engine, temp_path=str(tmp_path))      # writes the cache
            assert tuple(VD_w[k] for k in KEYS) == want and VD_w['bbs'] == VD['bbs']
        assert os.path.isfile(cache)
        stamp = os.path.getmtime(cache)
        VD_c, _ = S.smart_vid_crop(v, CP, save_vid=False, engine=engine, temp_path=str(tmp_path))          # served from it
        assert os.path.getmtime(cache) == stamp
        for other in (VD_s, VD_c):
            assert tuple(other[k] for k in KEYS) == want
            assert (other['fbb_w'], other['fbb_h']) == (fw, fh) and other['bbs'] == VD['bbs']
            assert np.array_equal(other['border_f_col'], f_col) and np.array_equal(other['border_f_row'], f_row)


def _same_video(a, b, ratios):
    for r in ratios:
        va, vb = a[r][0], b[r][0]
        assert tuple(va[k] for k in KEYS) == tuple(vb[k] for k in KEYS)
        assert np.array_equal(va['border_f_col'], vb['border_f_col']) and np.array_equal(va['border_f_row'], vb['border_f_row'])
        assert (va['fbb_w'], va['fbb_h']) == (vb['fbb_w'], vb['fbb_h'])
        assert va['bbs'] == vb['bbs'] and va['dx'] == vb['dx'] and va['dy'] == vb['dy']
        assert va['dxs_smooth'] == vb['dxs_smooth']
        assert a[r][1]['info'] == b[r][1]['info']
        assert a[r][1]['pixels_per_grey_level_at_threshold'] == b[r][1]['pixels_per_grey_level_at_threshold']
    assert torch.equal(a[ratios[0]][0]['smaps_dev'], b[ratios[0]][0]['smaps_dev'])


def _job_videos():
    """Bordered and border-free videos of different lengths (5 ... 40 selected frames: chunks hold several videos)."""
    return [_barred_video(100, 11, 'letterbox', 50, trans=[0, 41, 100]), _barred_video(60, 21, 'full', 0),
            _barred_video(25, 12, 'pillarbox', 90), _barred_video(190, 22, 'full', 0, trans=[0, 7, 100, 190]),
            _barred_video(45, 13, 'letterbox', 70, trans=[0, 20, 45]), _barred_video(130, 14, 'pillarbox', 120),
            _barred_video(33, 23, 'full', 0)]


@pytest.mark.parametrize('read_batch,lanes', [(None, 2), (7, 1), (None, 1)], ids=['in_place', 'tmp_branch', 'one_lane'])
def test_packed_job_with_borders_equals_every_video_alone(engine, synthetic_sd, tmp_path, read_batch, lanes):
    """crop_videos(packed=True): every video equals smart_vid_crop_ratios on it alone; some have borders, some none.  read_batch
    = 7 puts an all-zero row (the reference's off-by-one per read batch) after every few maps, so chunks of 32 frames straddle
    zero rows and _Lane.step goes through its `tmp` branch."""
    CP0 = S.sc_init_crop_params()
    vids = _job_videos()
    f_col, f_row, h, w = _raw_profile(engine, vids[0], CP0)
    tb = _t_border_for('letterbox', f_col, f_row)
    assert 0 < tb < 255
    CP = dict(CP0, t_border=tb)
    if read_batch:
        CP['read_batch'] = read_batch
    ratios = ('1:3', '3:1')
    seq = [S.smart_vid_crop_ratios(v, CP, ratios, engine=engine) for v in vids]
    brd = [tuple(s['1:3'][0][k] for k in KEYS) for s in seq]
    print('t_border %d, borders per video %s' % (tb, brd))
    assert any(any(b) for b in brd) and any(not any(b) for b in brd)
    for s in seq:                                          # the second ratio re-uses the video's borders
        assert tuple(s['3:1'][0][k] for k in KEYS) == tuple(s['1:3'][0][k] for k in KEYS)
    seen_tmp = []
    if read_batch:
        step = scheduler._Lane.step

        def spy(self):
            before = None if self.pipe is None else (self.frames_done, self.rows_called)
            ok = step(self)
            if before is not None and self.frames_done > before[0]:
                rows = self.row_of_frame[before[0]:self.frames_done]
                seen_tmp.append(int(rows[-1]) - int(rows[0]) + 1 != len(rows))
            return ok
        scheduler._Lane.step = spy
    try:
        par = S.crop_videos([(lambda v=v: v) for v in vids], CP, ratios, workers=lanes, state_dict=synthetic_sd, packed=True)
    finally:
        if read_batch:
            scheduler._Lane.step = step
    if read_batch:
        assert any(seen_tmp)                               # zero rows fell inside a chunk: the `tmp` branch ran
    for a, b in zip(seq, par):
        _same_video(a, b, ratios)
    # the result files carry the bordered windows
    i = next(k for k, b in enumerate(brd) if any(b))
    VD = par[i]['1:3'][0]
    fn = S.write_results(str(tmp_path), 'vid%d' % i, '1:3', VD, par[i]['1:3'][1])
    lines = [tuple(int(x) for x in ln.split(',')) for ln in open(fn).read().split()]
    assert lines == [tuple(b) for b in VD['bbs']]
    t, b, l, r = brd[i]
    assert all(x1 >= l and y1 >= t and x2 <= vids[i]['w'] - r and y2 <= vids[i]['h'] - b for x1, y1, x2, y2 in lines)


def test_render_of_a_bordered_result_never_shows_a_bar(engine):
    """Bars of 54 rows = exactly 21 map rows (360 / 140 * 21), so map rows 0..20 and 119..139 lie wholly inside a bar.  The
    synthetic checkpoint does not map black to dark (it sees the bar's edge), so t_border is the brightest of those rows: the
    restatement then counts at least 21 rows on either side, int((360 / 140) * 21) = 54 pixels, the whole bar."""
    CP0 = S.sc_init_crop_params()
    bar, k = 54, 21
    v = _barred_video(100, 11, 'letterbox', bar, trans=[0, 41, 100])
    f_col, f_row, h, w = _raw_profile(engine, v, CP0)
    assert (h, w) == (140, 250)
    tb = int(max(f_col[:k].max(), f_col[-k:].max()))
    print('t_border %d  f_col[:24] %s  f_col[-24:] %s' % (tb, f_col[:24], f_col[-24:]))
    assert 0 < tb < 255
    want = _np_borders(f_col, f_row, tb, h, w, v['h'], v['w'])
    assert want[0] >= bar and want[1] >= bar
    assert v['frames'][:, bar:v['h'] - bar].reshape(100, v['h'] - 2 * bar, -1).max(2).min() > 0     # only the bars have black rows
    for ratio in ('1:3', '3:1'):
        VD, _ = S.smart_vid_crop(v, dict(CP0, t_border=tb, out_ratio=ratio), save_vid=False, engine=engine)
        assert tuple(VD[key] for key in KEYS) == want
        crops = render.render_video(v, VD, engine=engine)
        assert crops.shape == (VD['fc'], VD['fbb_h'], VD['fbb_w'], 3)
        for i, (x1, y1, x2, y2) in enumerate(VD['bbs']):
            assert np.array_equal(crops[i], v['frames'][i, y1:y2, x1:x2])
        bb = VD['bbs_np']
        assert (bb[:, 1] >= bar).all() and (bb[:, 3] <= v['h'] - bar).all()
        assert crops.reshape(VD['fc'], VD['fbb_h'], -1).max(2).min() > 0           # no row of a bar in any crop


def test_border_off_allocates_no_profile_and_launches_what_the_census_call_launches(engine, synthetic_sd):
    """t_border = -1: the lanes hold no profile tensor and the network's last class ('smooth') records, per pass, exactly the
    launches of a saliency(threshold=t, census=c) call in this process; with t_border set it is the same count (the banded
    kernel takes the place of the flat one)."""
    CP = S.sc_init_crop_params()
    fr = torch.from_numpy(synth.blob_frames(32, 140, 250, seed=4)).cuda()
    c = torch.zeros((32, 4), dtype=torch.int32, device='cuda')
    engine.profile_enable('smooth')
    try:
        engine.saliency(fr, threshold=CP['t_threshold'], census=c)
        _, per_pass = engine.profile_read()
        engine.saliency(fr, threshold=CP['t_threshold'], census=c, profile=torch.zeros((32, 390), dtype=torch.int32, device='cuda'))
        _, per_pass_profile = engine.profile_read()
    finally:
        engine.profile_enable(None)
    assert per_pass >= 1 and per_pass_profile == per_pass
    vids = [_barred_video(64, 30 + k, 'full', 0) for k in range(3)]
    for tb in (-1, 40):
        js = scheduler.JobScheduler(dict(CP, t_border=tb), ('1:3',), lanes=1, state_dict=synthetic_sd)
        seen = []
        alloc = scheduler._Lane._alloc

        def spy(self, *a, **k):
            alloc(self, *a, **k)
            seen.append(self)
        scheduler._Lane._alloc = spy
        eng = js.engines[0]
        passes = []
        sal = eng.saliency
        eng.saliency = lambda *a, **k: (passes.append(1), sal(*a, **k))[1]
        try:
            eng.profile_enable('smooth')
            js.run(vids)
            _, launches = eng.profile_read()
            eng.profile_enable(None)
        finally:
            scheduler._Lane._alloc = alloc
            del eng.saliency
            js.close()
        assert seen and passes
        for lane in seen:
            assert (lane.profile is None and lane.profile_tmp is None) if tb == -1 else tuple(lane.profile.shape) == (lane.cap, 390)
        assert launches == per_pass * len(passes), (tb, launches, len(passes))
