"""A state-dict with the layout of the REFERENCE model class — all 834 entries, including rnn.*, post_rnn.* and the
three other domains, in the class's order (tests/golden/checkpoint_layout.npz, tools/make_golden_checkpoint_layout.py) —
goes through the product's loader/folder, and the oracle driven by that same dict reproduces the reference forward
stored with the layout.  This is what dropping in the real weights_best.pth exercises."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_state_dict_loads_and_matches(golden_dir):
    sys.path.insert(0, ROOT)
    from tools.make_golden_checkpoint_layout import layout_state_dict, network_input, unpack
    from oracle import unisal_ref as U
    from retargetvid_amd import weights
    torch.set_num_threads(1)
    g = np.load(os.path.join(golden_dir, 'checkpoint_layout.npz'))
    sd = layout_state_dict(*unpack(g))                       # non-trivial BN statistics
    ref = torch.from_numpy(g['ref'])
    assert len(sd) == 834 and any(k.startswith('rnn.') for k in sd)
    layers = weights.fold_state_dict(sd)                     # torch tensors, extra keys ignored
    blob = weights.pack_blob(layers)
    assert len(layers) == 67 and len(blob) > 12_000_000         # stem + 50 backbone + f18 + 4 skip + gaussians + 8 decoder + adapt + smoothing
    x = network_input()
    pre = U.forward_logits(weights.to_numpy_state_dict(sd), x, (140, 250))
    got = torch.log_softmax(pre.reshape(1, -1), 1).reshape(140, 250)
    assert (got - ref).abs().max() < 1e-5
