"""tests/golden/checkpoint_layout.npz: the state-dict LAYOUT of the reference model class (all 834 entries: key, shape,
dtype, in the class's own order -- rnn.*, post_rnn.* and the three other domains included) and the reference model's
static SALICON forward on a checkpoint of that layout, so that tests/test_reference_checkpoint_layout.py runs anywhere.

The checkpoint's values are a recipe of the test (layout_state_dict below, shared with it): the static slice from
weights.make_reference_init_state_dict(7), every BatchNorm running statistic re-drawn (N(0, 0.1) / U(0.7, 1.3)), the
tensors off the static path U(-0.1, 0.1), the counters 0.  The reference model code is imported in the build container
through tools/ref_import.py.

Stored: keys / dtypes (str), ndims and the flattened shapes (int64), the input (seeded N(0, 1), 1 x 3 x 256 x 416) is
regenerated from its seed, `ref` = the reference's log-softmax map (140 x 250, float32, one CPU thread).

Run from the repo root:  python tools/make_golden_checkpoint_layout.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retargetvid_amd import weights          # noqa: E402

X_SEED = 5


def layout_state_dict(keys, shapes, dtypes):
    """The checkpoint of the test: torch tensors under the reference class's keys, in its order."""
    ri = weights.make_reference_init_state_dict(7)
    rng = np.random.RandomState(3)
    sd = {}
    for key, shape, dt in zip(keys, shapes, dtypes):
        shape = tuple(int(s) for s in shape)
        if np.dtype(dt).kind in 'iu':
            v = np.zeros(shape, dt)
        elif key.endswith('.running_mean'):
            v = rng.normal(0, 0.1, shape)
        elif key.endswith('.running_var'):
            v = rng.uniform(0.7, 1.3, shape)
        elif key in ri:
            v = ri[key]
        else:
            v = rng.uniform(-0.1, 0.1, shape)
        sd[key] = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dt).reshape(shape)))
    return sd


def network_input():
    return torch.from_numpy(np.random.RandomState(X_SEED).standard_normal((1, 3, 256, 416)).astype(np.float32))


def unpack(g):
    """npz -> (keys, shapes, dtypes)"""
    dims = g['ndims']
    flat = g['shapes']
    at = np.concatenate([[0], np.cumsum(dims)])
    return [str(k) for k in g['keys']], [flat[at[i]:at[i + 1]] for i in range(len(dims))], [str(d) for d in g['dtypes']]


def main():
    from tools.ref_import import load_reference_unisal
    torch.set_num_threads(1)
    net, _ = load_reference_unisal()
    ref_sd = net.state_dict()
    keys = list(ref_sd)
    shapes = [tuple(v.shape) for v in ref_sd.values()]
    dtypes = [str(v.numpy().dtype) for v in ref_sd.values()]
    sd = layout_state_dict(keys, shapes, dtypes)
    net.load_state_dict(sd, strict=True)
    net.eval()
    with torch.no_grad():
        ref = net(network_input()[:, None], target_size=(140, 250), source='SALICON', static=True)[0, 0, 0]
    out = os.path.join(ROOT, 'tests', 'golden', 'checkpoint_layout.npz')
    np.savez_compressed(out, keys=np.array(keys), dtypes=np.array(dtypes), ndims=np.array([len(s) for s in shapes], np.int64),
                        shapes=np.array([d for s in shapes for d in s], np.int64), ref=ref.numpy().astype(np.float32))
    print(out, len(keys), 'entries')


if __name__ == '__main__':
    main()
