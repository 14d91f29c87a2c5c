"""-m gpu: rendering the retargeted frames (svc_render_crops_u8, ops.Engine.render_crops, render.render_video and the
save_vid door of smart_vid_crop) against numpy slices and the INTER_LINEAR oracle, bit for bit."""
import os
import pickle

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import cv_ref, pipeline_ref as P
from retargetvid_amd import ingest, render, smartVidCrop as S, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]


def _frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def _boxes(n, h, w, bw, bh, seed):
    """n windows of bw x bh: the four corners of the frame first (every edge touched), then odd / random origins."""
    rng = np.random.RandomState(seed)
    xs = [0, w - bw, 0, w - bw] + [int(v) | 1 if w > bw else 0 for v in rng.randint(0, w - bw + 1, n)]
    ys = [0, 0, h - bh, h - bh] + [int(v) for v in rng.randint(0, h - bh + 1, n)]
    xs = [min(x, w - bw) for x in xs[:n]]
    ys = ys[:n]
    return np.array([[x, y, x + bw, y + bh] for x, y in zip(xs, ys)], np.int32)


def _slices(frames, boxes):
    return np.stack([f[y1:y2, x1:x2] for f, (x1, y1, x2, y2) in zip(frames, boxes)])


def test_copy_path_is_exact(engine):
    for (h, w), sizes in (((360, 640), ((121, 360), (203, 360), (17, 5), (15, 9), (640, 360), (1, 1))),
                          ((1080, 1920), ((607, 1080), (608, 1080), (1919, 1077)))):
        frames = _frames(6, h, w, seed=h)
        d = torch.from_numpy(frames).cuda()
        for bw, bh in sizes:
            boxes = _boxes(6, h, w, bw, bh, seed=bw)
            exp = _slices(frames, boxes)
            got = engine.render_crops(d, torch.from_numpy(boxes).cuda())
            assert np.array_equal(got.cpu().numpy(), exp), (h, w, bw, bh)
            got = engine.render_crops(d, boxes, bgr=True)
            assert np.array_equal(got.cpu().numpy(), exp[..., ::-1]), (h, w, bw, bh, 'bgr')


def test_copy_path_unaligned_buffers(engine):
    """Frames / output that do not start on 16 bytes take the per-pixel kernel: same bytes."""
    frames = _frames(3, 36, 64, seed=1)
    raw = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), frames.ravel()])).cuda()
    d = raw[1:].view(3, 36, 64, 3)
    boxes = _boxes(3, 36, 64, 33, 20, seed=2)
    out = torch.empty(1 + 3 * 20 * 33 * 3, dtype=torch.uint8, device='cuda')[1:].view(3, 20, 33, 3)
    got = engine.render_crops(d, boxes, out=out, bgr=True)
    assert np.array_equal(got.cpu().numpy(), _slices(frames, boxes)[..., ::-1])


def test_resize_path_matches_the_oracle(engine):
    cases = (((360, 640), (203, 360), (1920, 1080)),        # non-integer upscale (a 9:16 window of 640x360 to 1080x1920)
             ((360, 640), (320, 180), (90, 160)),           # exact 2:1 downscale
             ((2160, 3840), (1215, 2160), (1080, 608)),     # non-integer downscale (4K 9:16 window)
             ((360, 640), (301, 77), (50, 333)))            # anisotropic
    for (h, w), (bw, bh), (oh, ow) in cases:
        frames = _frames(3, h, w, seed=bw)
        boxes = _boxes(3, h, w, bw, bh, seed=oh)
        d = torch.from_numpy(frames).cuda()
        got = engine.render_crops(d, boxes, out_hw=(oh, ow)).cpu().numpy()
        gotb = engine.render_crops(d, boxes, out_hw=(oh, ow), bgr=True).cpu().numpy()
        for i, (x1, y1, x2, y2) in enumerate(boxes):
            exp = cv_ref.resize_linear_u8(np.ascontiguousarray(frames[i, y1:y2, x1:x2]), oh, ow)
            assert np.array_equal(got[i], exp), ((h, w), (bw, bh), (oh, ow), i)
            assert np.array_equal(gotb[i], exp[..., ::-1])


def _vd(n, h, w, bw, bh, seed):
    return dict(fc=n, bbs_np=_boxes(n, h, w, bw, bh, seed).astype(np.int64))


def test_render_video_every_container(engine):
    n, h, w = 45, 360, 640
    VD = _vd(n, h, w, 121, 360, seed=5)
    lazy = synth.LazyBlobVideo(n + 3, h, w, seed=4)
    frames = lazy.select(range(n + 3)).cpu().numpy()
    exp = _slices(frames[:n], VD['bbs_np'])
    pinned = torch.from_numpy(frames).pin_memory()
    for name, cont in (('numpy', frames), ('pinned', pinned), ('cuda', torch.from_numpy(frames).cuda()), ('lazy', lazy)):
        got = render.render_video(cont, VD, engine=engine, chunk=16)
        assert np.array_equal(got, exp), name
        seen = []
        render.render_video(dict(frames=cont), VD, engine=engine, chunk=16, sink=lambda c: seen.append(c.copy()))
        assert [len(c) for c in seen] == [16, 16, 13] and np.array_equal(np.concatenate(seen), exp), name
    got = render.render_video(frames, VD, engine=engine, out_size=(200, 300), bgr=True)
    for i, (x1, y1, x2, y2) in enumerate(VD['bbs_np']):
        assert np.array_equal(got[i], cv_ref.resize_linear_u8(np.ascontiguousarray(frames[i, y1:y2, x1:x2]), 300, 200)[..., ::-1])
    resident = synth.ResidentBlobVideo(n, list(range(n)), h, w, seed=4)
    with pytest.raises(ValueError):
        render.render_video(synth.HostSelectedVideo(resident), VD, engine=engine)
    with pytest.raises(ValueError):
        render.render_video(frames[:n - 1], VD, engine=engine)


def _video(n, seed, trans):
    return dict(fr=30.0, frame_count=n, w=640, h=360, frames=synth.blob_frames(n, 360, 640, seed=seed),
                trans_inds=trans)


def test_pickle_mode_writes_the_reference_crops(engine, synthetic_sd, tmp_path):
    torch.set_num_threads(8)
    for ratio, seed, trans in (('1:3', 3, [0, 40, 90]), ('3:1', 4, [0, 90])):
        video = _video(90, seed, trans)
        p = str(tmp_path / ('clip_%s.pkl' % ratio.replace(':', 'x')))
        with open(p, 'wb') as fp:
            pickle.dump(video, fp)
        CP = S.sc_init_crop_params()
        CP['out_ratio'] = ratio
        VD, res = S.smart_vid_crop(p, CP, final_vid_fn='x', engine=engine)
        assert 't_render' in res and not os.path.exists('x')
        with open(p.replace('.pkl', '_sc.pkl'), 'rb') as fp:
            got = pickle.load(fp)
        frames = video['frames']
        exp = [np.ascontiguousarray(frames[i][:, :, ::-1])[y1:y2, x1:x2] for i, (x1, y1, x2, y2) in enumerate(VD['bbs'])]
        assert len(got) == len(exp) == 90
        assert all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, exp))
        ref = P.smart_vid_crop(video, dict(P.init_crop_params(), out_ratio=ratio), synthetic_sd)
        exp_ref = [np.ascontiguousarray(frames[i][:, :, ::-1])[y1:y2, x1:x2] for i, (x1, y1, x2, y2) in enumerate(ref['bbs'])]
        assert all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, exp_ref))


class _Recorder:
    def __init__(self, log, path, fr, size):
        self.log = log
        log.update(args=(path, fr, size), frames=[], released=0)

    def write(self, f):
        self.log['frames'].append(np.array(f))

    def release(self):
        self.log['released'] += 1


def test_writer_hook(engine, tmp_path):
    video = _video(40, 7, [0, 40])
    CP = S.sc_init_crop_params()
    CP['out_ratio'] = '9:16'
    log = {}
    S.set_video_writer(lambda path, fr, size: _Recorder(log, path, fr, size))
    try:
        VD, res = S.smart_vid_crop(video, CP, final_vid_fn='out_clip', engine=engine)
        assert log['args'] == ('out_clip', 30.0, (VD['fbb_w'], VD['fbb_h'])) and log['released'] == 1
        assert np.array_equal(np.stack(log['frames']), _slices(video['frames'], VD['bbs_np'])) and 't_render' in res
        S.smart_vid_crop(video, CP, final_vid_fn='out_clip', engine=engine, out_size=(108, 192))
        assert log['args'][2] == (108, 192) and log['frames'][0].shape == (192, 108, 3) and len(log['frames']) == 40
        S.set_video_writer(ingest.write_frames_pillow)
        out_dir = str(tmp_path / 'frames_out')
        VD, _ = S.smart_vid_crop(video, CP, final_vid_fn=out_dir, engine=engine)
        back = ingest.read_frames_pillow(out_dir, fr=30.0)
        assert np.array_equal(back['frames'], _slices(video['frames'], VD['bbs_np']))
    finally:
        S.set_video_writer(None)


def test_streams(engine):
    """Four renders on four streams at once, beside a saliency pass on a fifth: the single-stream bytes."""
    frames = _frames(8, 1080, 1920, seed=9)
    d = torch.from_numpy(frames).cuda()
    jobs = [(_boxes(8, 1080, 1920, 608, 1080, seed=s), None if s % 2 else (1920, 1080), bool(s & 2)) for s in range(4)]
    solo = [engine.render_crops(d, b, out_hw=o, bgr=g).cpu().numpy() for b, o, g in jobs]
    small = torch.from_numpy(synth.blob_frames(8, 140, 250, seed=1)).cuda()
    maps_solo = engine.saliency(small).cpu().numpy()
    boxes = [torch.from_numpy(b).cuda() for b, _, _ in jobs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(5)]
    outs = []
    for k, (s, (b, o, g)) in enumerate(zip(streams, jobs)):
        with torch.cuda.stream(s):
            outs.append(engine.render_crops(d, boxes[k], out_hw=o, bgr=g))
    with torch.cuda.stream(streams[4]):
        maps = engine.saliency(small)
    torch.cuda.synchronize()
    for k in range(4):
        assert np.array_equal(outs[k].cpu().numpy(), solo[k]), k
    assert np.array_equal(maps.cpu().numpy(), maps_solo)
