"""-m gpu: NV12 input (svc_resize_frames_nv12, svc_render_crops_nv12 and every door that takes a video dict with
pix_fmt='nv12') against the RGB path on the converted frames, bit for bit.  Every expected value comes from
nv12_ref.nv12_to_rgb (the fixed-point BT.601 formula in numpy) of the NV12 bytes actually fed; nothing has a tolerance."""
import pickle

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import nv12_ref
from oracle import cv_ref
from retargetvid_amd import ops, render, smartVidCrop as S, synth, weights

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]


def _random_nv12(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h * 3 // 2, w)).astype(np.uint8)


def _structured_nv12(n, h, w, seed):
    return nv12_ref.rgb_to_nv12(synth.blob_frames(n, h, w, seed=seed))


def _boxes(n, h, w, bw, bh, seed):
    """tests/test_gpu_render.py's windows: the four corners of the frame first (every edge touched), then odd x origins and
    random (odd and even) y origins."""
    rng = np.random.RandomState(seed)
    xs = [0, w - bw, 0, w - bw] + [int(v) | 1 if w > bw else 0 for v in rng.randint(0, w - bw + 1, n)]
    ys = [0, 0, h - bh, h - bh] + [int(v) for v in rng.randint(0, h - bh + 1, n)]
    xs = [min(x, w - bw) for x in xs[:n]]
    ys = ys[:n]
    return np.array([[x, y, x + bw, y + bh] for x, y in zip(xs, ys)], np.int32)


def _slices(frames, boxes):
    return np.stack([f[y1:y2, x1:x2] for f, (x1, y1, x2, y2) in zip(frames, boxes)])


def test_every_triple_through_the_copy_path(engine):
    """One 4096 x 4096 frame holding all 2^24 (Y, U, V) triples, rendered with the full-frame window."""
    f = nv12_ref.all_triples_frame()[None]
    exp = nv12_ref.nv12_to_rgb(f, 4096, 4096)
    d = torch.from_numpy(f).cuda()
    box = np.array([[0, 0, 4096, 4096]], np.int32)
    got = engine.render_crops(d, box, pix_fmt='nv12').cpu().numpy()
    assert np.array_equal(got, exp)
    got = engine.render_crops(d, box, bgr=True, pix_fmt='nv12').cpu().numpy()
    assert np.array_equal(got, exp[..., ::-1])


@pytest.mark.parametrize('src,dst', [((360, 640), (140, 250)), ((360, 640), (27, 48)), ((1080, 1920), (140, 250)),
                                     ((1080, 1920), (27, 48)), ((2160, 3840), (140, 250)), ((2160, 3840), (27, 48)),
                                     ((640, 360), (250, 140)), ((360, 640), (180, 320)), ((36, 64), (140, 250)), ((2, 2), (1, 1))])
def test_downscale_equals_the_rgb_path_and_the_oracle(engine, src, dst):
    (h, w), (sh, sw) = src, dst
    n = 2 if h >= 1080 else 3
    for kind, nv in (('random', _random_nv12(n, h, w, seed=h + sw)), ('structured', _structured_nv12(n, h, w, seed=w + sh))):
        rgb = nv12_ref.nv12_to_rgb(nv, h, w)
        got = engine.resize_frames(torch.from_numpy(nv).cuda(), sh, sw, pix_fmt='nv12').cpu().numpy()
        via_rgb = engine.resize_frames(torch.from_numpy(rgb).cuda(), sh, sw).cpu().numpy()
        assert got.shape == (n, sh, sw, 3)
        assert np.array_equal(got, via_rgb), (kind, 'rgb path')
        for i in range(n):
            assert np.array_equal(got[i], cv_ref.resize_linear_u8(rgb[i], sh, sw)), (kind, 'oracle', i)


def test_downscale_of_an_unaligned_buffer(engine):
    nv = _random_nv12(3, 36, 64, seed=3)
    raw = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), nv.ravel()])).cuda()
    got = engine.resize_frames(raw[1:].view(3, 54, 64), 14, 25, pix_fmt='nv12').cpu().numpy()
    rgb = nv12_ref.nv12_to_rgb(nv, 36, 64)
    assert np.array_equal(got, np.stack([cv_ref.resize_linear_u8(f, 14, 25) for f in rgb]))


def test_copy_path_is_exact(engine):
    for (h, w), sizes in (((360, 640), ((121, 360), (203, 360), (17, 5), (15, 9), (640, 360), (1, 1), (16, 2), (33, 3))),
                          ((1080, 1920), ((607, 1080), (608, 1080), (1919, 1077)))):
        nv = _random_nv12(6, h, w, seed=h)
        frames = nv12_ref.nv12_to_rgb(nv, h, w)
        d = torch.from_numpy(nv).cuda()
        for bw, bh in sizes:
            boxes = _boxes(6, h, w, bw, bh, seed=bw)
            exp = _slices(frames, boxes)
            got = engine.render_crops(d, torch.from_numpy(boxes).cuda(), pix_fmt='nv12')
            assert np.array_equal(got.cpu().numpy(), exp), (h, w, bw, bh)
            got = engine.render_crops(d, boxes, bgr=True, pix_fmt='nv12')
            assert np.array_equal(got.cpu().numpy(), exp[..., ::-1]), (h, w, bw, bh, 'bgr')
    # a picture whose width is no multiple of 16 (row starts at every even phase), windows at every x and y parity
    h, w = 38, 70
    nv = _random_nv12(8, h, w, seed=11)
    frames = nv12_ref.nv12_to_rgb(nv, h, w)
    d = torch.from_numpy(nv).cuda()
    for bw, bh in ((17, 9), (33, 21), (70, 38), (69, 37)):
        boxes = np.array([[x, y, x + bw, y + bh] for x, y in zip(np.arange(8) % (w - bw + 1), (np.arange(8) // 2) % (h - bh + 1))], np.int32)
        assert np.array_equal(engine.render_crops(d, boxes, pix_fmt='nv12').cpu().numpy(), _slices(frames, boxes)), (bw, bh)


def test_copy_path_unaligned_buffers(engine):
    """Frames / output that do not start on 16 bytes take the per-pixel kernel: same bytes."""
    nv = _random_nv12(3, 36, 64, seed=1)
    frames = nv12_ref.nv12_to_rgb(nv, 36, 64)
    raw = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), nv.ravel()])).cuda()
    d = raw[1:].view(3, 54, 64)
    boxes = _boxes(3, 36, 64, 33, 20, seed=2)
    out = torch.empty(1 + 3 * 20 * 33 * 3, dtype=torch.uint8, device='cuda')[1:].view(3, 20, 33, 3)
    got = engine.render_crops(d, boxes, out=out, bgr=True, pix_fmt='nv12')
    assert np.array_equal(got.cpu().numpy(), _slices(frames, boxes)[..., ::-1])
    got = engine.render_crops(d, boxes, out_hw=(40, 50), pix_fmt='nv12').cpu().numpy()      # the resize path's bytewise staging
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        assert np.array_equal(got[i], cv_ref.resize_linear_u8(np.ascontiguousarray(frames[i, y1:y2, x1:x2]), 40, 50))


def test_resize_path_matches_the_oracle(engine):
    cases = (((360, 640), (203, 360), (1920, 1080)),        # non-integer upscale (a 9:16 window of 640x360 to 1080x1920)
             ((360, 640), (320, 180), (90, 160)),           # exact 2:1 downscale
             ((2160, 3840), (1215, 2160), (1080, 608)),     # non-integer downscale (4K 9:16 window)
             ((360, 640), (301, 77), (50, 333)))            # anisotropic
    for (h, w), (bw, bh), (oh, ow) in cases:
        nv = _random_nv12(3, h, w, seed=bw)
        frames = nv12_ref.nv12_to_rgb(nv, h, w)
        boxes = _boxes(3, h, w, bw, bh, seed=oh)
        d = torch.from_numpy(nv).cuda()
        got = engine.render_crops(d, boxes, out_hw=(oh, ow), pix_fmt='nv12').cpu().numpy()
        gotb = engine.render_crops(d, boxes, out_hw=(oh, ow), bgr=True, pix_fmt='nv12').cpu().numpy()
        via_rgb = engine.render_crops(torch.from_numpy(frames).cuda(), boxes, out_hw=(oh, ow)).cpu().numpy()
        assert np.array_equal(got, via_rgb)
        for i, (x1, y1, x2, y2) in enumerate(boxes):
            exp = cv_ref.resize_linear_u8(np.ascontiguousarray(frames[i, y1:y2, x1:x2]), oh, ow)
            assert np.array_equal(got[i], exp), ((h, w), (bw, bh), (oh, ow), i)
            assert np.array_equal(gotb[i], exp[..., ::-1])


def test_c_abi_refuses_odd_pictures(engine):
    d = torch.zeros((1, 54, 64), dtype=torch.uint8, device='cuda')
    out = torch.zeros((1, 14, 25, 3), dtype=torch.uint8, device='cuda')
    box = torch.zeros((1, 4), dtype=torch.int32, device='cuda')
    lib, vp = engine.lib, lambda t: t.data_ptr()
    assert lib.svc_resize_frames_nv12(engine._h, vp(d), 1, 36, 64, vp(out), 14, 25, None) == 0
    assert lib.svc_resize_frames_nv12(engine._h, vp(d), 1, 35, 64, vp(out), 14, 25, None) == -1
    assert lib.svc_resize_frames_nv12(engine._h, vp(d), 1, 36, 63, vp(out), 14, 25, None) == -1
    assert lib.svc_resize_frames_nv12(engine._h, None, 0, 36, 64, None, 14, 25, None) == 0          # n = 0: a no-op
    assert lib.svc_render_crops_nv12(engine._h, vp(d), 1, 36, 64, vp(box), 25, 14, vp(out), 14, 25, 0, None) == 0
    assert lib.svc_render_crops_nv12(engine._h, vp(d), 1, 35, 64, vp(box), 25, 14, vp(out), 14, 25, 0, None) == -1
    assert lib.svc_render_crops_nv12(engine._h, vp(d), 1, 36, 62 + 1, vp(box), 25, 14, vp(out), 14, 25, 0, None) == -1
    assert lib.svc_render_crops_nv12(engine._h, vp(d), 1, 36, 64, vp(box), 25, 14, vp(out), 14, 25, 2, None) == -1   # unknown flag
    assert lib.svc_render_crops_nv12(engine._h, vp(d), 1, 36, 64, vp(box), 65, 14, vp(out), 14, 25, 0, None) == -1   # window wider than the picture
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        engine.resize_frames(torch.zeros((1, 55, 64), dtype=torch.uint8, device='cuda'), 14, 25, pix_fmt='nv12')
    engine.profile_enable('resize')
    engine.resize_frames(d, 14, 25, pix_fmt='nv12')
    assert engine.profile_read()[1] == 1                       # counted under SVC_K_RESIZE
    engine.profile_enable('render')
    engine.render_crops(d, np.array([[1, 1, 26, 15]], np.int32), pix_fmt='nv12')
    assert engine.profile_read()[1] == 1                       # ... and SVC_K_RENDER
    engine.profile_enable(None)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _pair(n, seed, trans, h=360, w=640, cut=None):
    """A synthetic video as NV12 and as its converted RGB twin (the same pictures, byte for byte, after conversion)."""
    rgb = synth.blob_frames(n, h, w, seed=seed)
    if cut is not None:
        rgb[cut:] = rgb[cut:][:, ::-1]                        # a hard cut
    nv = nv12_ref.rgb_to_nv12(rgb)
    base = dict(fr=30.0, frame_count=n, w=w, h=h)
    if trans is not None:
        base['trans_inds'] = trans
    return dict(base, frames=nv, pix_fmt='nv12'), dict(base, frames=nv12_ref.nv12_to_rgb(nv, h, w))


def _same(a, b):
    assert np.array_equal(a['smaps'], b['smaps'])
    assert a['dx'] == b['dx'] and a['dy'] == b['dy']
    assert np.array_equal(a['bbs_np'], b['bbs_np']) and a['true_inds'] == b['true_inds']


def test_smart_vid_crop_gives_the_rgb_twins_results(engine):
    torch.set_num_threads(8)
    nv, rgb = _pair(120, 5, [0, 50, 120], cut=50)
    for CP in (S.sc_init_crop_params(), S.sc_init_crop_params(use_best_settings=True)):
        CP['out_ratio'] = '9:16'
        want, _ = S.smart_vid_crop(rgb, CP, save_vid=False, engine=engine)
        got, _ = S.smart_vid_crop(nv, CP, save_vid=False, engine=engine)
        assert got['smaps'].any()
        _same(got, want)
        got, _ = S.smart_vid_crop(nv, CP, save_vid=False, engine=engine, stream_batch=16)
        want_s, _ = S.smart_vid_crop(rgb, CP, save_vid=False, engine=engine, stream_batch=16)
        _same(got, want_s)
        assert np.array_equal(got['bbs_np'], want['bbs_np'])
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    want, _ = S.smart_vid_crop(rgb, CP, save_vid=False, engine=engine)
    for name, cont in (('pinned', torch.from_numpy(nv['frames']).pin_memory()), ('cuda', torch.from_numpy(nv['frames']).cuda())):
        got, _ = S.smart_vid_crop(dict(nv, frames=cont), CP, save_vid=False, engine=engine)
        _same(got, want)
    with pytest.raises(ValueError):                           # RGB frames under an NV12 label: refused by the plan
        S.smart_vid_crop(dict(rgb, pix_fmt='nv12'), CP, save_vid=False, engine=engine)


def test_shot_detection_sees_equal_bytes(engine):
    from retargetvid_amd import transnetv1_handler as Hd
    net = Hd.ShotTransNet(Hd.ShotTransNetParams(), weights=weights.make_transnet_state_dict(0))
    try:
        nv, rgb = _pair(150, 9, None, h=90, w=160, cut=60)
        nv['fr'] = rgb['fr'] = 25.0
        CP = dict(S.sc_init_crop_params(), read_batch=64, out_ratio='1:3', hdbscan_min=5)
        a = S.detect_shots(nv['frames'], 25.0, CP, net=net, pix_fmt='nv12')
        b = S.detect_shots(rgb['frames'], 25.0, CP, net=net)
        assert np.array_equal(a['trans_probs'], b['trans_probs']) and np.array_equal(a['segmentation'], b['segmentation'])
        want, _ = S.smart_vid_crop(rgb, CP, save_vid=False, engine=engine, shot_net=net)
        got, _ = S.smart_vid_crop(nv, CP, save_vid=False, engine=engine, shot_net=net)
        assert np.array_equal(got['trans_probs'], want['trans_probs'])
        _same(got, want)
    finally:
        net.close()


def test_crop_videos_with_mixed_formats_equals_the_single_runs(engine, synthetic_sd):
    torch.set_num_threads(8)
    pairs = [_pair(60 + 15 * k, 20 + k, [0, 30 + 5 * k, 60 + 15 * k]) for k in range(4)]
    vids = [p[k & 1] for k, p in enumerate(pairs)]            # nv12, rgb, nv12, rgb
    assert [v.get('pix_fmt') for v in vids] == ['nv12', None, 'nv12', None]
    CP = S.sc_init_crop_params()
    ratios = ('1:3', '3:1')
    par = S.crop_videos(vids, CP, ratios, workers=2, state_dict=synthetic_sd)
    twins = S.crop_videos([p[1] for p in pairs], CP, ratios, workers=2, state_dict=synthetic_sd)
    for v, p, t in zip(vids, par, twins):
        for r in ratios:
            one, _ = S.smart_vid_crop(v, dict(CP, out_ratio=r), save_vid=False, engine=engine)
            assert np.array_equal(p[r][0]['bbs_np'], one['bbs_np']) and p[r][0]['dx'] == one['dx']
            assert np.array_equal(p[r][0]['bbs_np'], t[r][0]['bbs_np']) and np.array_equal(p[r][0]['smaps'], t[r][0]['smaps'])


def test_render_video_and_pickle_mode(engine, tmp_path):
    torch.set_num_threads(8)
    nv, rgb = _pair(45, 4, [0, 45])
    n, h, w = 45, 360, 640
    VD = dict(fc=n, bbs_np=_boxes(n, h, w, 121, 360, seed=5).astype(np.int64))
    exp = _slices(rgb['frames'], VD['bbs_np'])
    f = nv['frames']
    for name, cont in (('numpy', f), ('pinned', torch.from_numpy(f).pin_memory()), ('cuda', torch.from_numpy(f).cuda())):
        got = render.render_video(dict(nv, frames=cont), VD, engine=engine, chunk=16)
        assert np.array_equal(got, exp), name
        got = render.render_video(cont, VD, engine=engine, chunk=16, pix_fmt='nv12')
        assert np.array_equal(got, exp), name
    got = render.render_video(nv, VD, engine=engine, out_size=(200, 300), bgr=True)
    assert np.array_equal(got, render.render_video(rgb, VD, engine=engine, out_size=(200, 300), bgr=True))
    for i, (x1, y1, x2, y2) in enumerate(VD['bbs_np']):
        assert np.array_equal(got[i], cv_ref.resize_linear_u8(np.ascontiguousarray(rgb['frames'][i, y1:y2, x1:x2]), 300, 200)[..., ::-1])
    assert np.array_equal(render.render_video(rgb, VD, engine=engine), exp)      # (the render feed goes back to RGB staging)
    # the .pkl mode: BGR crops of native size, from an NV12 pickle and from its RGB twin
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    out = {}
    for name, video in (('nv12', nv), ('rgb', rgb)):
        p = str(tmp_path / ('clip_%s.pkl' % name))
        with open(p, 'wb') as fp:
            pickle.dump(video, fp)
        VD2, res = S.smart_vid_crop(p, CP, final_vid_fn='x', engine=engine)
        with open(p.replace('.pkl', '_sc.pkl'), 'rb') as fp:
            out[name] = (pickle.load(fp), VD2['bbs'])
    assert out['nv12'][1] == out['rgb'][1] and len(out['nv12'][0]) == 45
    assert all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(out['nv12'][0], out['rgb'][0]))
    assert all(np.array_equal(g, rgb['frames'][i][y1:y2, x1:x2, ::-1]) for i, (g, (x1, y1, x2, y2)) in enumerate(zip(*out['nv12'])))
    # the writer mode
    log = []

    class Writer:
        def write(self, fr):
            log.append(np.array(fr))

        def release(self):
            pass

    S.set_video_writer(lambda path, fr, size: Writer())
    try:
        VD3, _ = S.smart_vid_crop(nv, CP, final_vid_fn='out_clip', engine=engine)
        assert np.array_equal(np.stack(log), _slices(rgb['frames'], VD3['bbs_np']))
    finally:
        S.set_video_writer(None)


def test_feature_cache_keys_on_the_format(engine, tmp_path):
    nv, rgb = _pair(40, 6, [0, 40])
    CP = dict(S.sc_init_crop_params(), out_ratio='1:3')
    S.smart_vid_crop(dict(rgb, name='clip'), CP, save_vid=False, engine=engine, temp_path=str(tmp_path))
    with open(str(tmp_path / 'clip.pkl'), 'rb') as fp:
        assert pickle.load(fp)['cache_key']['pix_fmt'] == 'rgb24'
    S.smart_vid_crop(dict(nv, name='clip'), CP, save_vid=False, engine=engine, temp_path=str(tmp_path))
    with open(str(tmp_path / 'clip.pkl'), 'rb') as fp:
        assert pickle.load(fp)['cache_key']['pix_fmt'] == 'nv12'       # written again under the other format


def test_host_feed_staging_is_sized_by_the_frames_bytes(engine):
    """Half the pinned and device staging per frame: the NV12 slots hold k frames of h * 3 / 2 * w bytes."""
    feed = S._HostFeed(engine)
    nv = _random_nv12(5, 360, 640, seed=8)
    got = feed.downscale(nv, [0, 2, 4], 140, 250, pix_fmt='nv12').cpu().numpy()
    assert tuple(feed.staged[0].shape[1:]) == (540, 640) and tuple(feed.pinned[0].shape[1:]) == (540, 640)
    rgb = nv12_ref.nv12_to_rgb(nv, 360, 640)
    assert np.array_equal(got, np.stack([cv_ref.resize_linear_u8(rgb[i], 140, 250) for i in (0, 2, 4)]))
    got = feed.downscale(rgb, [0, 2, 4], 140, 250).cpu().numpy()
    assert tuple(feed.staged[0].shape[1:]) == (360, 640, 3)
    assert np.array_equal(got, np.stack([cv_ref.resize_linear_u8(rgb[i], 140, 250) for i in (0, 2, 4)]))
