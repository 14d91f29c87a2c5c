"""-m gpu: frames.FrameSource reads every kind of container to the same bytes.  70 frames of a 64 x 36 picture (at this size the
host feed stages 32 frames per slot: 70 selected frames cross a chunk boundary and come back to a slot of the double
buffer) in both formats, packed and pitched, in every container; the reference side of every comparison is the engine's
packed device-tensor entry (Engine.resize_frames / render_crops) on frames gathered on the host."""
import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
import nv12_ref
from retargetvid_amd import ops, smartVidCrop as S
from retargetvid_amd.frames import FrameSource

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

N, H, W = 70, 36, 64
SH, SW = 14, 25
SELECTIONS = (range(N), range(0, N, 3), [5, 5, 40, 39, 69, 0, 33, 34, 35, 2, 68], [])
PITCHED = dict(nv12=dict(pitch=128, chroma_offset=128 * H), rgb24=dict(pitch=200))
STRIDE = dict(nv12=9216, rgb24=200 * H)           # (the NV12 surfaces keep a gap behind their chroma plane)


class Gen:
    """An on-device generator over a CUDA tensor; with_index: select takes the frame numbers as a device tensor."""

    def __init__(self, dev_frames, with_index):
        self.t, self.h, self.w, self.accepts_device_index = dev_frames, H, W, with_index
        if not with_index:
            self.select = lambda idx: self._select(idx)

    def __len__(self):
        return N

    def _select(self, idx, index=None):
        if index is None:
            index = torch.as_tensor(np.asarray(list(idx), np.int64), device=self.t.device)
        return self.t[index]

    select = _select


class Selected:
    """synth.HostSelectedVideo's interface: the frames in pinned memory in another order, rows(idx) finds them."""

    def __init__(self, frames):
        order = np.random.RandomState(3).permutation(N)
        self.h, self.w = H, W
        self.pinned = torch.from_numpy(np.ascontiguousarray(frames[order])).pin_memory()
        self.row = {int(f): r for r, f in enumerate(order)}

    def __len__(self):
        return N

    def rows(self, idx):
        return [self.row[int(i)] for i in idx]


def _pitch(packed, fmt):
    """The packed frames as [N, frame_stride] rows of PITCHED[fmt], every padding byte 0xFF."""
    lay = PITCHED[fmt]
    rows = packed.reshape(N, -1, W if fmt == 'nv12' else 3 * W)          # [N, plane rows, row bytes]
    buf = np.full((N, STRIDE[fmt]), 0xFF, np.uint8)
    for r in range(rows.shape[1]):
        at = r * lay['pitch'] if r < H else lay['chroma_offset'] + (r - H) * lay['pitch']
        buf[:, at:at + rows.shape[2]] = rows[:, r]
    return buf


@pytest.fixture(scope='module', params=ops.PIX_FMTS)
def case(request, engine):
    """(fmt, packed host frames, packed device frames, the reference small frames per selection, [(name, FrameSource)])."""
    fmt = request.param
    rgb = np.random.RandomState(7).randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    packed = rgb if fmt == 'rgb24' else nv12_ref.rgb_to_nv12(rgb)
    dev = torch.from_numpy(packed).cuda()
    pitched = _pitch(packed, fmt)
    L = ops.frame_layout(fmt, H, W, PITCHED[fmt], pitched.shape[1])
    assert (L.frame_stride, L.extent < L.frame_stride) == ((9216, True) if fmt == 'nv12' else (7200, True))
    conts = [('numpy', packed, None), ('host tensor', torch.from_numpy(packed.copy()), None),
             ('pinned', torch.from_numpy(packed).pin_memory(), None), ('cuda', dev.clone(), None),
             ('generator, device index', Gen(dev, True), None), ('generator', Gen(dev, False), None), ('selected', Selected(packed), None),
             ('pitched numpy', pitched, L), ('pitched pinned', torch.from_numpy(pitched).pin_memory(), L),
             ('pitched cuda', torch.from_numpy(pitched).cuda(), L)]
    want = [engine.resize_frames(torch.from_numpy(packed[np.asarray(list(idx), np.int64)]).cuda(), SH, SW, fmt) for idx in SELECTIONS]
    sources = [(name, FrameSource.of(c, fmt, lay)) for name, c, lay in conts]
    kinds = [s.kind for _, s in sources]
    assert kinds == ['host', 'host', 'pinned', 'device', 'generator', 'generator', 'selected', 'host', 'pinned', 'device']
    assert all((s.n, s.h, s.w, s.pix_fmt) == (N, H, W, fmt) for _, s in sources)
    return fmt, packed, dev, want, sources


def test_small_gives_the_packed_bytes_from_every_container(engine, case):
    fmt, packed, dev, want, sources = case
    for name, src in sources:
        for idx, exp in zip(SELECTIONS, want):
            got = src.small(engine, idx, SH, SW)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(idx), SH, SW, 3), (name, idx)
            assert torch.equal(got, exp), (fmt, name, idx)
    assert want[0].any() and not torch.equal(want[0][0], want[0][1])


def test_chunks_give_the_packed_crops_from_every_container(engine, case):
    fmt, packed, dev, want, sources = case
    boxes = np.array([[x, y, x + 20, y + 16] for x, y in (((3 * i) % (W - 20), i % (H - 16)) for i in range(N))], np.int32)
    exp = engine.render_crops(dev, boxes, pix_fmt=fmt)
    assert exp.any()
    for name, src in sources:
        if src.kind == 'selected':
            with pytest.raises(ValueError, match='needs every frame'):
                src.chunks(engine, N, 16, lambda staged, s: pytest.fail('no chunk may arrive'))
            continue
        seen = []
        src.chunks(engine, N, 16, lambda staged, s: seen.append((s, staged.clone())))       # (a staged chunk is valid until its work has run)
        assert [s for s, _ in seen] == list(np.cumsum([0] + [int(c.shape[0]) for _, c in seen[:-1]])), name
        whole = torch.cat([c for _, c in seen])
        assert whole.shape[0] == N and all(c.device == engine.device for _, c in seen), name
        got = engine.render_crops(whole, boxes, pix_fmt=fmt, layout=src.layout)
        assert torch.equal(got, exp), (fmt, name)


def test_detect_shots_sees_the_same_frames_in_device_and_host_memory(engine, case):
    """The CUDA container (a slice per read batch) against the numpy container (the host feed), through a stub network that
    records what it is shown."""
    fmt, packed, dev, want, sources = case

    class Net:
        eng, predict_frames = engine, None               # (video_transition_probs reads the attribute, predict_video is what runs)

        def __init__(self):
            self.shown = []

        def predict_video(self, arr, keep=None):
            self.shown.append(arr.cpu())
            return arr.reshape(arr.shape[0], -1).float().mean(1).div(255.0).cpu().numpy()
    CP = dict(S.sc_init_crop_params(), read_batch=32)
    nets, out = [Net(), Net()], []
    for net, cont in zip(nets, (dev, packed)):
        out.append(S.detect_shots(cont, 25.0, CP, net=net, trans_threshold=0.45, pix_fmt=fmt))
    assert len(nets[0].shown) == len(nets[1].shown) == 3 and nets[0].shown[0].any()
    assert all(torch.equal(a, b) for a, b in zip(nets[0].shown, nets[1].shown))
    assert np.array_equal(out[0]['trans_probs'], out[1]['trans_probs']) and len(out[0]['trans_probs']) == N
    assert np.array_equal(out[0]['segmentation'], out[1]['segmentation']) and out[0]['trans_inds'] == out[1]['trans_inds']
    # ... and what the network was shown is the packed frames at its input size
    from retargetvid_amd import transnetv1_handler as T
    small = engine.resize_frames(dev, T.ShotTransNetParams.INPUT_HEIGHT, T.ShotTransNetParams.INPUT_WIDTH, fmt).cpu()
    overlap = int(25.0 - 5)
    assert torch.equal(torch.cat([a[overlap:overlap + 32] for a in nets[0].shown])[:N], small)
