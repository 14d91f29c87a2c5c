"""No GPU: frames.FrameSource.of -- what kind of container holds a video's frames, its format, layout and size, resolved once and
without device work, for every container x format x layout, from a video dict and from a bare container; the feature
cache's entries; detect_shots' refusal of a container that holds only selected frames."""
import numpy as np
import pytest
import torch

from retargetvid_amd import ops, smartVidCrop as S
from retargetvid_amd.frames import FrameSource

H, W, N = 36, 64, 4
PITCHED = dict(nv12=dict(pitch=128, chroma_offset=128 * H), rgb24=dict(pitch=200))
STRIDE = dict(nv12=9216, rgb24=200 * H)


class Gen:
    """An on-device generator: frames on demand, none is asked for here."""
    h, w = H, W

    def __len__(self):
        return N

    def select(self, idx):
        raise AssertionError('no frame may be asked for')


class Selected:
    """synth.HostSelectedVideo's interface (.pinned, .rows): 2 of the video's N frames, no pinning without a device."""
    h, w = H, W

    def __init__(self, shape):
        self.pinned = torch.zeros((2,) + shape, dtype=torch.uint8)

    def __len__(self):
        return N

    def rows(self, idx):
        raise AssertionError('no frame may be asked for')


def _containers(shape):
    z = np.zeros((N,) + shape, np.uint8)
    return (('numpy', 'host', z), ('list', 'host', [f for f in z]), ('tensor', 'host', torch.from_numpy(z)),
            ('generator', 'generator', Gen()), ('selected', 'selected', Selected(shape)))


def _seen(src):
    return src.kind, src.n, src.h, src.w, src.pix_fmt, src.layout is None


@pytest.mark.parametrize('fmt', ops.PIX_FMTS)
@pytest.mark.parametrize('pitched', [False, True])
def test_every_container_format_and_layout(fmt, pitched):
    shape = (STRIDE[fmt],) if pitched else ops.frame_shape(fmt, H, W)
    lay = PITCHED[fmt] if pitched else None
    L = ops.frame_layout(fmt, H, W, lay, STRIDE[fmt]) if pitched else None
    for name, kind, cont in _containers(shape):
        if pitched and kind == 'generator':
            for video in (dict(frames=cont, w=W, h=H, pix_fmt=fmt, layout=lay), ):
                with pytest.raises(ValueError, match=r'\.select'):
                    FrameSource.of(video)
            with pytest.raises(ValueError, match=r'\.select'):
                FrameSource.of(cont, fmt, L)
            continue
        want = (kind, N, H, W, fmt, not pitched)
        video = dict(frames=cont, fr=25.0, frame_count=N, w=W, h=H, pix_fmt=fmt, layout=lay)
        src = FrameSource.of(video)
        assert _seen(src) == want and src.layout == L, name
        assert FrameSource.of(src) is src
        assert _seen(FrameSource.of(video, 'nv12' if fmt == 'rgb24' else 'rgb24')) == want, name      # a dict's own entries win
        assert _seen(FrameSource.of(cont, fmt, L)) == want and FrameSource.of(cont, fmt, L).layout == L, name       # the bare form
        if pitched:
            assert _seen(FrameSource.of(cont, layout=L)) == want, name          # a FrameLayout names its format
        else:
            no_size = dict(frames=cont, pix_fmt=fmt)                           # h, w from the container's shape (the objects' h, w)
            assert _seen(FrameSource.of(no_size)) == want, name
        if kind == 'host':
            assert src.frames.shape == (N,) + shape and (name != 'list' or isinstance(src.frames, np.ndarray))
        else:
            assert src.frames is cont
        assert (S.video_pix_fmt(video), S.video_layout(video)) == (fmt, L)
    assert _seen(FrameSource.of(np.zeros((N, H, W, 3), np.uint8))) == ('host', N, H, W, 'rgb24', True)      # the defaults


def test_refusals_keep_their_types():
    z = np.zeros((N, H, W, 3), np.uint8)
    for bad in (z.astype(np.float32), z[..., :2], z[0]):
        with pytest.raises(TypeError, match='uint8 .n,h,w,3. RGB'):
            FrameSource.of(bad)
        with pytest.raises(TypeError, match='uint8 .n,h,w,3. RGB'):
            FrameSource.of(dict(frames=bad, w=W, h=H))
    with pytest.raises(TypeError, match='nv12 frames must be uint8'):
        FrameSource.of(np.zeros((N, 54, W), np.int16), 'nv12')
    with pytest.raises(ValueError, match='nv12 frames of a 64 x 36 picture are uint8 .n, 54, 64., not'):
        FrameSource.of(dict(frames=Selected((H, W, 3)), w=W, h=H, pix_fmt='nv12'))
    with pytest.raises(ValueError):
        FrameSource.of(np.zeros((N, 54, W), np.uint8), 'nv21')
    with pytest.raises(ValueError, match='pix_fmt'):
        FrameSource.of(dict(frames=np.zeros((N, 54, W), np.uint8), w=W, h=H, pix_fmt='nv21'))
    L = ops.frame_layout('nv12', H, W, PITCHED['nv12'], 9216)
    for bad in (np.zeros((N, 9216), np.int8), np.zeros((N, 9216 + 64), np.uint8)):
        with pytest.raises(ValueError, match='frames with this layout are uint8 .n, 9216., not'):
            FrameSource.of(bad, 'nv12', L)
    with pytest.raises(ValueError, match='are uint8 .n, frame_stride., not .4, 54, 64.'):
        FrameSource.of(np.zeros((N, 54, W), np.uint8), 'nv12', L)


def test_a_dict_without_frames_still_has_its_key():
    """smart_vid_crop's feature cache answers for a dict whose frames are gone; planning such a dict is a TypeError."""
    video = dict(frames=None, fr=25.0, frame_count=N, w=W, h=H, pix_fmt='nv12', trans_inds=[0, N])
    src = FrameSource.of(video)
    assert (src.kind, src.n, src.key()) == (None, None, dict(pix_fmt='nv12'))
    with pytest.raises(TypeError):
        S.plan_video(video, S.sc_init_crop_params())


def test_key_is_the_feature_caches():
    CP = S.sc_init_crop_params()
    eng = type('E', (), dict(weights_id=1))()
    base = dict(fr=25.0, frame_count=N, w=W, h=H, pix_fmt='nv12', trans_inds=[0, N])
    packed = dict(base, frames=np.zeros((N, 54, W), np.uint8))
    pitched = dict(base, frames=np.zeros((N, 9216), np.uint8), layout=PITCHED['nv12'])
    rgb = dict(fr=25.0, frame_count=N, w=W, h=H, trans_inds=[0, N], frames=np.zeros((N, H, W, 3), np.uint8))
    assert FrameSource.of(packed).key() == dict(pix_fmt='nv12') and FrameSource.of(rgb).key() == dict(pix_fmt='rgb24')
    assert FrameSource.of(pitched).key() == dict(pix_fmt='nv12', layout=('nv12', H, W, 9216, 128, 128 * H, 128))
    for video in (packed, pitched, rgb):
        full, key = S.feature_cache_key(video, CP, eng), FrameSource.of(video).key()
        assert {k: full[k] for k in key} == key and ('layout' in full) == (video is pitched)
        assert list(full)[-len(key):] == list(key)                # (the entries' order is part of the pickled key)


def test_detect_shots_refuses_selected_frames_before_the_network():
    class Net:
        def __getattr__(self, name):
            raise AssertionError('the network may not be touched')
    for frames in (Selected((H, W, 3)), FrameSource.of(Selected((H, W, 3)))):
        with pytest.raises(ValueError, match='only the frames the ingest selected'):
            S.detect_shots(frames, 25.0, net=Net())
    with pytest.raises(ValueError, match='only the frames the ingest selected'):
        FrameSource.of(Selected((H, W, 3))).whole()
