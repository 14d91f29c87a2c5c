"""-m gpu: a plain `bench.py --gpus 1` run (no --full) times one region of exactly --steps steps, prints the headline
fields and, with --dump-outputs, writes what the timed path computed in its last step: the centres, crop windows and
filtered maps of that step's batch must be those of the plain call on the same frames in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned_outputs, poisoned_workspaces  # noqa: F401  (fixtures)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('poisoned_outputs', 'poisoned_workspaces')]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_last_step(engine, tmp_path):
    out = str(tmp_path / 'outputs')
    steps = 6                                              # four batches in flight: the last step is slot 1's batch
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
           '--dump-outputs', out]
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in d, k
    assert d['steps'] == steps and d['config']['repeats']['regions'] == 1 and d['ms_per_step'] > 0
    assert abs(d['value'] - 32 * 1e3 / d['ms_per_step']) < 1e-2 * d['value']
    assert d['roofline'] is None and d['cpu_baseline'] is None and d['config']['config3'] is None   # --full only

    xy = np.load(os.path.join(out, 'centres.npy'))
    boxes = np.load(os.path.join(out, 'boxes.npy'))
    maps = np.load(os.path.join(out, 'maps.npy'))
    assert xy.dtype == np.float64 and xy.shape == (32, 2)
    assert boxes.dtype == np.float64 and boxes.shape == (32, 4)
    assert maps.dtype == np.float32 and maps.shape == (32, 140, 250)
    assert sum(a.nbytes for a in (xy, boxes, maps)) <= 64 << 20
    assert (boxes == np.round(boxes)).all() and boxes.min() >= 0 and boxes[:, 2].max() <= 640 and boxes[:, 3].max() <= 360

    # the same batch (slot k = (steps - 1) % 4: seed 100 + 1000 k, bench.py's blob sizes) through the plain call here
    from retargetvid_amd import smartVidCrop as S, synth
    k = (steps - 1) % 4
    frames = synth.blob_frames(32, 360, 640, seed=100 + 1000 * k, n_blobs=2, sigma=(30.0, 44.0))
    CP = S.sc_init_crop_params()
    flags = np.zeros(32, np.uint8)
    flags[:2] = 1
    small = engine.resize_frames(torch.from_numpy(frames).cuda(), 140, 250)
    m = engine.saliency(small)
    engine.threshold_(m, CP['t_threshold'])
    exp_xy = engine.cluster_center_(m, flags, CP).cpu().numpy()
    assert np.array_equal(xy, exp_xy, equal_nan=True)
    assert np.array_equal(maps, m.cpu().numpy().astype(np.float32))
