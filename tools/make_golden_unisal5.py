"""tests/golden/unisal_golden5.npz: the REFERENCE model code (imported in the build container through tools/ref_import.py) at the
eight network input sizes that golden2-4 do not reach.  get_optimal_out_size selects one of eleven sizes from the saliency-map
shape; golden2-4 cover 256x416, 288x384 and 416x256.  Here one map shape per remaining size:

  166x250 -> 288x416 (3:2)   200x250 -> 320x384 (5:4)   230x250 -> 320x352   249x249 -> 320x320 (1:1)
  250x230 -> 352x320         250x200 -> 384x320 (4:5)   250x187 -> 384x288 (3:4)   250x166 -> 416x288 (2:3)

Checkpoints: nc (weights.make_synthetic_state_dict(3, carrier=False)), ri (weights.make_reference_init_state_dict(7) with the
BatchNorm statistics of golden2), tl and tl2 (weights.make_trained_like_state_dict, variants 1 and 2).  Two frames per geometry,
synth.blob_frames(2, h, w, seed=SEED[geometry]); the frames are not stored, their SHA-256 is (frames_sha256_<geom>), and the tests
regenerate them and check it.

Stored per (checkpoint, geometry), small enough for the repository (fp32 maps hardly compress; the full set would be ~5 MB):
  adapt_<ck>_<geom>_0   the adaptation output of frame 0 (NH/8 x NW/8) on grid(NH/8, NW/8, 2): every other row and column and
                        the last ones
  logp_<ck>_<geom>_0    the log-softmax map of frame 0 on grid(h, w): every 8th row and column and the last ones (borders included)
  u8_<ck>_<geom>_<i>    the u8 map (train.py:1270-1274) of both frames: whole for the peaky tl / tl2 maps (FULL_U8, they compress
                        to a few kB), on grid(h, w, U8_STEP) for the diffuse nc / ri maps (every other row and column: ~15 000 pixels,
                        enough for the tests' fraction-of-pixels gates); every u8 map 2-D difference coded (encode_u8 /
                        decode_u8: exact, a third smaller once compressed)
Pre-processing as in tools/make_golden_unisal2.py (Pillow LANCZOS + ToTensor + Normalize).  Single-threaded, so that a rerun gives the
same arrays.

Run from the repo root:  python tools/make_golden_unisal5.py"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from retargetvid_amd import synth, weights                  # noqa: E402

GEOMS = {'3x2': (166, 250), '5x4': (200, 250), '11x10': (230, 250), '1x1': (249, 249),
         '10x11': (250, 230), '4x5': (250, 200), '3x4': (250, 187), '2x3': (250, 166)}
NET = {'3x2': (288, 416), '5x4': (320, 384), '11x10': (320, 352), '1x1': (320, 320),
       '10x11': (352, 320), '4x5': (384, 320), '3x4': (384, 288), '2x3': (416, 288)}
SEED = {g: 500 + i for i, g in enumerate(GEOMS)}
CKS = ('nc', 'ri', 'tl', 'tl2')
FULL_U8 = ('tl', 'tl2')
U8_STEP = 2
N = 2


def grid(h, w, step=8):
    """Rows and columns of the stored samples of an h x w map: every step-th and the last."""
    return np.unique(np.r_[0:h:step, h - 1]), np.unique(np.r_[0:w:step, w - 1])


def encode_u8(a):
    """u8 map -> its differences along both axes (uint8, wrapping): smooth maps compress better."""
    return np.diff(np.diff(a, axis=1, prepend=np.uint8(0)), axis=0, prepend=np.uint8(0))


def decode_u8(d):
    return np.cumsum(np.cumsum(d, axis=0, dtype=np.uint8), axis=1, dtype=np.uint8)


def on_grid(a, h, w, step=8):
    rows, cols = grid(h, w, step)
    return np.ascontiguousarray(a[np.ix_(rows, cols)])


def frames_of(gname):
    h, w = GEOMS[gname]
    return synth.blob_frames(N, h, w, seed=SEED[gname])


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def checkpoint(ck, golden_dir):
    if ck == 'nc':
        return weights.make_synthetic_state_dict(3, carrier=False)
    if ck == 'ri':
        g2 = np.load(os.path.join(golden_dir, 'unisal_golden2.npz'))
        return weights.make_reference_init_state_dict(7, {k[3:]: g2[k] for k in g2.files if k.startswith('bn/')})
    return weights.make_trained_like_state_dict(golden_dir, variant=1 if ck == 'tl' else 2)


def main():
    # the tests import GEOMS / SEED / N from here: Pillow and the reference code only where the golden is made
    from tools.make_golden_unisal2 import load, prep
    from tools.ref_import import load_reference_unisal
    torch.set_num_threads(1)
    golden_dir = os.path.join('tests', 'golden')
    net, _ = load_reference_unisal()
    out = {}
    for gname in GEOMS:
        out['frames_sha256_' + gname] = np.array(sha256(frames_of(gname)))
    for ck in CKS:
        load(net, checkpoint(ck, golden_dir))
        net.eval()
        taps = {}
        hook = net.adaptation_salicon.register_forward_hook(lambda m, i, o: taps.__setitem__('adapt', o))
        with torch.no_grad():
            for gname, (h, w) in GEOMS.items():
                frames = frames_of(gname)
                nh, nw = NET[gname]
                for i in range(N):
                    pred = net(prep(frames[i], nh, nw)[None, None], target_size=(h, w), source='SALICON', static=True)
                    assert taps['adapt'].shape[-2:] == (nh // 8, nw // 8)
                    smap = torch.squeeze(pred[:, 0, ...].exp()).numpy()
                    smap = (smap / np.amax(smap)) * 255.0                     # train.py:1270-1274
                    tag = '%s_%s_%d' % (ck, gname, i)
                    u8 = smap.astype('uint8')
                    out['u8_' + tag] = encode_u8(u8 if ck in FULL_U8 else on_grid(u8, h, w, U8_STEP))
                    assert np.array_equal(decode_u8(out['u8_' + tag]), u8 if ck in FULL_U8 else on_grid(u8, h, w, U8_STEP))
                    if i == 0:
                        out['logp_' + tag] = on_grid(pred[0, 0, 0].numpy(), h, w)
                        out['adapt_' + tag] = on_grid(taps['adapt'][0, 0].numpy(), nh // 8, nw // 8, 2)
                print(ck, gname, 'u8 map: nonzero %.3f, >=120: %.3f' % ((u8 > 0).mean(), (u8 >= 120).mean()), flush=True)
        hook.remove()
    path = os.path.join(golden_dir, 'unisal_golden5.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path))


if __name__ == '__main__':
    main()
