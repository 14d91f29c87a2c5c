"""No GPU: the definition of the renderer's NV12 output (nv12_out_ref.rgb_to_nv12_fixed, the formula of include/svc.h) and
everything the NV12-output doors decide on the host -- the ValueErrors raised before any device work, and the raw writer."""
import numpy as np
import pytest
import torch

import nv12_out_ref
import nv12_ref
from retargetvid_amd import ingest, ops, render, smartVidCrop as S

BARS = (((0, 0, 0), (16, 128, 128)), ((255, 0, 0), (82, 90, 240)), ((0, 255, 0), (145, 54, 34)), ((255, 255, 0), (210, 16, 146)),
        ((0, 0, 255), (41, 240, 110)), ((255, 0, 255), (107, 202, 222)), ((0, 255, 255), (170, 166, 16)),
        ((255, 255, 255), (235, 128, 128)))


@pytest.mark.parametrize('rgb,yuv', BARS)
def test_colour_bars(rgb, yuv):
    """The eight corner colours give the BT.601 colour-bar values."""
    out = nv12_out_ref.rgb_to_nv12_fixed(np.broadcast_to(np.array(rgb, np.uint8), (2, 2, 3)).copy())
    assert out.shape == (3, 2)
    assert (out[:2] == yuv[0]).all() and tuple(out[2]) == yuv[1:]


def test_layout_and_the_block_sum():
    """Luma per pixel, chroma from the sum of the 2 x 2 block, pairs interleaved in row oh + j; a batch is its frames."""
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, (3, 6, 10, 3)).astype(np.uint8)
    out = nv12_out_ref.rgb_to_nv12_fixed(rgb)
    assert out.shape == (3, 9, 10) and out.dtype == np.uint8
    r, g, b = (int(v) for v in rgb[1, 3, 7])
    assert out[1, 3, 7] == (269484 * r + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20
    sr, sg, sb = (int(v) for v in rgb[1, 4:6, 2:4].reshape(4, 3).astype(np.int64).sum(0))
    assert out[1, 6 + 2, 2] == (-155188 * sr - 305135 * sg + 460324 * sb + (128 << 22) + (1 << 21)) >> 22
    assert out[1, 6 + 2, 3] == (460324 * sr - 385875 * sg - 74448 * sb + (128 << 22) + (1 << 21)) >> 22
    assert np.array_equal(nv12_out_ref.rgb_to_nv12_fixed(rgb[2]), out[2])


def test_output_ranges():
    """Y in 16..235, U and V in 16..240 -- on random full-range input and on blocks that mix the corner colours -- so the
    kernels need no clamp; the extremes are reached."""
    rng = np.random.RandomState(1)
    mixed = rng.choice(np.array([0, 255], np.uint8), size=(4, 64, 64, 3))
    flat = np.array([c for c, _ in BARS], np.uint8)[:, None, None, :].repeat(2, 1).repeat(2, 2)
    for rgb in (rng.randint(0, 256, (4, 64, 64, 3)).astype(np.uint8), mixed, flat):
        out = nv12_out_ref.rgb_to_nv12_fixed(rgb)
        h = rgb.shape[1]
        assert 16 <= out[:, :h].min() and out[:, :h].max() <= 235
        assert 16 <= out[:, h:].min() and out[:, h:].max() <= 240
    out = nv12_out_ref.rgb_to_nv12_fixed(flat)
    assert (out[:, :2].min(), out[:, :2].max(), out[:, 2:].min(), out[:, 2:].max()) == (16, 235, 16, 240)


def test_round_trip_of_flat_colours():
    """Decoding a flat colour with the NV12-input formula gives it back within 2 grey levels (measured over all 2^24 colours;
    here a 17-step lattice with both ends, all 2^16 colours of eight (r, g) planes, and a random draw)."""
    v = np.unique(np.r_[np.arange(0, 256, 17), 1, 254, 255]).astype(np.uint8)
    lattice = np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(-1, 3)
    b8 = np.array([0, 1, 37, 127, 128, 200, 254, 255], np.uint8)
    planes = np.stack(np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), b8, indexing='ij'), -1).reshape(-1, 3)
    rnd = np.random.RandomState(2).randint(0, 256, (1 << 16, 3)).astype(np.uint8)
    for colours in (lattice, planes, rnd):
        rgb = colours[:, None, None, :].repeat(2, 1).repeat(2, 2)          # every colour a frame of one 2 x 2 block
        back = nv12_ref.nv12_to_rgb(nv12_out_ref.rgb_to_nv12_fixed(rgb), 2, 2)
        assert np.abs(back.astype(np.int32) - rgb.astype(np.int32)).max() <= 2


def test_every_triple_frame_holds_every_triple_once():
    f = nv12_out_ref.every_rgb_triple_frame()
    assert f.shape == (4096, 4096, 3) and f.dtype == np.uint8
    key = (f[..., 0].astype(np.int64) << 16) | (f[..., 1].astype(np.int64) << 8) | f[..., 2]
    assert np.array_equal(np.sort(key.ravel()), np.arange(1 << 24))


def test_out_frame_shape():
    assert ops.OUT_FMTS == ('rgb24', 'nv12')
    assert ops.out_frame_shape('rgb24', 5, 7) == (5, 7, 3) and ops.out_frame_shape('rgb24', 5, 7, bgr=True) == (5, 7, 3)
    assert ops.out_frame_shape('nv12', 4, 6) == (6, 6)
    for bad in (dict(out_fmt='nv12', oh=5, ow=6), dict(out_fmt='nv12', oh=4, ow=7), dict(out_fmt='nv12', oh=0, ow=6),
                dict(out_fmt='nv12', oh=4, ow=6, bgr=True), dict(out_fmt='yuv420p', oh=4, ow=6)):
        with pytest.raises(ValueError):
            ops.out_frame_shape(**bad)


def _vd(n, bw, bh):
    return dict(fc=n, bbs_np=np.array([[1, 1, 1 + bw, 1 + bh]] * n, np.int64))


def test_render_video_refuses_before_any_device_work():
    frames = np.zeros((3, 12, 20, 3), np.uint8)
    with pytest.raises(ValueError, match='even out_size'):
        render.render_video(frames, _vd(3, 7, 6), out_fmt='nv12')                         # native size, odd window
    with pytest.raises(ValueError, match='even out_size'):
        render.render_video(frames, _vd(3, 8, 6), out_size=(8, 5), out_fmt='nv12')
    with pytest.raises(ValueError, match='out_fmt'):
        render.render_video(frames, _vd(3, 8, 6), out_fmt='yuv420p')
    with pytest.raises(ValueError, match='bgr'):
        render.render_video(frames, _vd(3, 8, 6), bgr=True, out_fmt='nv12')
    nv = np.zeros((3, 18, 20), np.uint8)
    with pytest.raises(ValueError, match='even out_size'):
        render.render_video(nv, _vd(3, 8, 6), out_size=(9, 6), pix_fmt='nv12', out_fmt='nv12')
    # an empty video is rendered without a device: the array has the format's shape
    assert render.render_video(frames, _vd(0, 0, 0), out_size=(8, 6), out_fmt='nv12').shape == (0, 9, 8)
    assert render.render_video(frames, _vd(0, 0, 0), out_size=(8, 6)).shape == (0, 6, 8, 3)


def test_render_crops_refuses_before_any_device_work():
    eng = object.__new__(ops.Engine)                 # (no handle: the checks below come before anything needs one)
    frames = torch.zeros((2, 12, 20, 3), dtype=torch.uint8)
    boxes = np.array([[0, 0, 7, 6], [1, 1, 8, 7]], np.int32)
    with pytest.raises(ValueError, match='even'):
        eng.render_crops(frames, boxes, out_fmt='nv12')
    with pytest.raises(ValueError, match='even'):
        eng.render_crops(frames, boxes, out_hw=(5, 8), out_fmt='nv12')
    with pytest.raises(ValueError, match='bgr'):
        eng.render_crops(frames, boxes, out_hw=(6, 8), bgr=True, out_fmt='nv12')
    with pytest.raises(ValueError, match='out_fmt'):
        eng.render_crops(frames, boxes, out_fmt='bgr24')
    with pytest.raises(TypeError):                   # an even size passes them and stops at the host tensor
        eng.render_crops(frames, boxes, out_hw=(6, 8), out_fmt='nv12')


def test_smart_vid_crop_refuses_before_any_work(tmp_path):
    video = dict(fr=25.0, frame_count=3, w=20, h=12, frames=np.zeros((3, 12, 20, 3), np.uint8), trans_inds=[0, 3])
    CP = S.sc_init_crop_params()
    made = []
    S.set_video_writer(lambda *a, **k: made.append(a))
    try:
        with pytest.raises(ValueError, match='pickle mode'):               # (the file does not exist: nothing opened it)
            S.smart_vid_crop(str(tmp_path / 'clip.pkl'), CP, final_vid_fn='x', out_pix_fmt='nv12')
        with pytest.raises(ValueError, match='out_fmt'):
            S.smart_vid_crop(video, CP, final_vid_fn=str(tmp_path / 'o'), out_pix_fmt='yuv420p')
        with pytest.raises(ValueError, match='even out_size'):
            S.smart_vid_crop(video, CP, final_vid_fn=str(tmp_path / 'o'), out_size=(9, 16), out_pix_fmt='nv12')
    finally:
        S.set_video_writer(None)
    assert not made and not list(tmp_path.iterdir())


@pytest.mark.parametrize('pix_fmt,shape', [('rgb24', (6, 8, 3)), ('nv12', (9, 8))])
def test_write_frames_raw(tmp_path, pix_fmt, shape):
    frames = np.random.RandomState(3).randint(0, 256, (5,) + shape).astype(np.uint8)
    path = str(tmp_path / ('clip.' + pix_fmt))
    w = ingest.write_frames_raw(path, 25.0, (8, 6), pix_fmt=pix_fmt)
    for f in frames[:4]:
        w.write(f)
    w.write(np.asfortranarray(frames[4]))             # (not contiguous: written in C order all the same)
    with pytest.raises(ValueError):
        w.write(frames[0][:-1])
    w.release()
    with open(path, 'rb') as fp:
        assert fp.read() == frames.tobytes()


def test_writers_and_formats(tmp_path):
    w = ingest.write_frames_raw(str(tmp_path / 'a'), 25.0, (8, 6))
    w.release()
    assert w.shape == (6, 8, 3) and w.pix_fmt == 'rgb24'          # the default
    for size in ((7, 6), (8, 5), (0, 2)):
        with pytest.raises(ValueError):
            ingest.write_frames_raw(str(tmp_path / 'b'), 25.0, size, pix_fmt='nv12')
    with pytest.raises(ValueError):
        ingest.write_frames_raw(str(tmp_path / 'b'), 25.0, (8, 6), pix_fmt='yuv420p')
    assert not (tmp_path / 'b').exists()
    with pytest.raises(ValueError, match='write_frames_raw'):
        ingest.write_frames_pillow(str(tmp_path / 'png'), 25.0, (8, 6), pix_fmt='nv12')
    assert not (tmp_path / 'png').exists()
