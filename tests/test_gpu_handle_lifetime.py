"""-m gpu: a handle owns everything it caches and shares none of it.  One list of calls reaches every cached table of a handle
-- the ingest's and the renderer's INTER_LINEAR tables, the LANCZOS tables and their upload, the tail's ring delta and shrink
tables, the network plan and its weight copies, the TransNet weights and workspace -- on the smallest shapes that do.  Engines are
created, used and closed in turn and side by side; every output is compared byte for byte (the centres too: NaN included).

Free device memory is not asserted on: other processes move that number.  That nothing leaks is what tests/test_devbuf_host.py
and the type itself state."""
import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
from oracle import pipeline_ref as P
from retargetvid_amd import ops, synth, weights
from retargetvid_amd import transnetv1_handler as TH

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]

CP = P.init_crop_params()
FLAGS = np.array([1, 0, 0, 0], np.uint8)
BOXES = np.array([[10, 20, 80, 110], [100, 30, 170, 120]], np.int32)        # two 70 x 90 windows of a 192 x 128 frame


@pytest.fixture(scope='module')
def inputs(synthetic_sd):
    rng = np.random.RandomState(5)
    return dict(sd=synthetic_sd, tsd=weights.make_transnet_state_dict(0),
                frames=torch.from_numpy(synth.blob_frames(2, 128, 192, seed=3)).cuda(),
                maps=torch.from_numpy(np.ascontiguousarray(synth.blob_frames(4, 64, 96, seed=4)[..., 0])).cuda(),
                window=torch.from_numpy(rng.randint(0, 256, (1, 12, 27, 48, 3)).astype(np.uint8)).cuda())


class Session:
    """An engine and its TransNet (the load), and the list of calls."""

    def __init__(self, inputs):
        self.eng = ops.Engine(inputs['sd'])
        self.net = TH.ShotTransNet(TH.ShotTransNetParams(), weights=inputs['tsd'], engine=self.eng)

    def run(self, inputs):
        eng, out = self.eng, {}
        out['small'] = eng.resize_frames(inputs['frames'], 64, 96)                      # the cv_tab entry of the ingest
        out['saliency'] = eng.saliency(out['small'])                                    # the plan, the weight copies
        for interp in ('linear', 'lanczos'):                                            # the window's cv_tab entry; lz_tab and its upload
            out[interp] = eng.render_crops(inputs['frames'], BOXES, out_hw=(45, 35), interp=interp)
        for factor in (1, 2):                                                           # the ring delta; the shrink tables and theirs
            maps = eng.threshold_(inputs['maps'].clone(), CP['t_threshold'])
            out['xy%d' % factor] = eng.cluster_center_(maps, FLAGS, dict(CP, resize_factor=factor))
            out['maps%d' % factor] = maps
        out['transnet'] = self.net.predict_raw_device(inputs['window'])
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().tobytes() for k, v in out.items()}

    def close(self):
        self.net.close()
        self.eng.close()


def _did_work(out):
    """The list is no row of empty calls: maps with salient pixels, a centre found at either factor, probabilities."""
    assert np.frombuffer(out['saliency'], np.uint8).max() > 0
    for factor in (1, 2):
        assert np.frombuffer(out['maps%d' % factor], np.uint8).any()
        assert np.isfinite(np.frombuffer(out['xy%d' % factor], np.float64)).any()
    assert np.isfinite(np.frombuffer(out['transnet'], np.float32)).all()
    assert out['linear'] != out['lanczos']


def test_teardown_and_recreate(inputs):
    outs = []
    for _ in range(3):
        s = Session(inputs)
        outs.append(s.run(inputs))
        s.close()
    _did_work(outs[0])
    for k in outs[0]:
        assert outs[2][k] == outs[0][k], k
        assert outs[1][k] == outs[0][k], k


def test_two_handles_at_once(inputs):
    a, b = Session(inputs), Session(inputs)
    out_a, before = a.run(inputs), b.run(inputs)
    a.close()
    after = b.run(inputs)                       # every table B cached is still B's own
    b.close()
    _did_work(before)
    for k in before:
        assert after[k] == before[k], k
        assert out_a[k] == before[k], k


def test_close_twice_and_close_unused(inputs):
    eng = ops.Engine(inputs['sd'])
    eng.close()                                 # never used
    eng.close()
    s = Session(inputs)
    s.run(inputs)
    s.eng.close()
    s.eng.close()
    assert not s.eng._h.value
