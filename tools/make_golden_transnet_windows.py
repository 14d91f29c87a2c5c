"""Record the reference's TransNet windowing (3rd_party_libs/transnetv1/transnetv1_handler.py:102-130, predict_video) ->
tests/golden/transnet_windows.npz.  BUILD CONTAINER ONLY: the reference tree is read here and nowhere at test time.

The handler imports ffmpeg, tensorflow and cv2 at module level (:1-4); none is needed for predict_video, so they are stubbed.  A
ShotTransNet is made without __init__ (no TensorFlow graph) and predict_raw is replaced by a recorder that returns a value encoding the
window and the slot (window * 1000 + slot), so the output names the (window, slot) each frame was taken from.

  python tools/make_golden_transnet_windows.py [--out tests/golden/transnet_windows.npz]

Per length n: win_<n> int32 [windows, 100] = the frame index in every slot (frames are their own index), out_<n> float64 [n] =
predict_video's output.  Written with fixed zip timestamps, so two runs give the same bytes."""
import argparse
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference/3rd_party_libs/transnetv1/transnetv1_handler.py'
LENGTHS = (1, 2, 24, 25, 26, 49, 50, 51, 74, 75, 76, 99, 100, 101, 149, 150, 151, 2037)


def load_reference_handler():
    for name in ('ffmpeg', 'tensorflow', 'cv2'):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location('ref_transnetv1_handler', REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def record(m, n):
    net = m.ShotTransNet.__new__(m.ShotTransNet)
    net.params = m.ShotTransNetParams()
    wins = []

    def predict_raw(frames):
        assert frames.shape[0] == 1 and frames.shape[1] == 100
        wins.append(frames[0, :, 0, 0, 0].astype(np.int64) + 256 * frames[0, :, 0, 0, 1].astype(np.int64))
        k = len(wins) - 1
        return (k * 1000 + np.arange(100, dtype=np.float64))[None]
    net.predict_raw = predict_raw
    fr = np.zeros((n, 27, 48, 3), np.uint8)                       # frame i carries its index in pixel (0, 0): i % 256, i // 256
    fr[:, 0, 0, 0] = np.arange(n) % 256
    fr[:, 0, 0, 1] = np.arange(n) // 256
    out = net.predict_video(fr)
    return np.stack(wins).astype(np.int32), np.asarray(out, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'transnet_windows.npz'))
    args = ap.parse_args()
    m = load_reference_handler()
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        z.writestr(zipfile.ZipInfo('lengths.npy', (1980, 1, 1, 0, 0, 0)), _npy(np.array(LENGTHS, np.int32)))
        for n in LENGTHS:
            w, o = record(m, n)
            for key, arr in (('win_%d' % n, w), ('out_%d' % n, o)):
                info = zipfile.ZipInfo(key + '.npy', (1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, _npy(arr))
    with open(args.out, 'wb') as f:
        f.write(buf.getvalue())
    print('%s: %d bytes, %d lengths' % (args.out, len(buf.getvalue()), len(LENGTHS)))


def _npy(arr):
    b = io.BytesIO()
    np.save(b, arr, allow_pickle=False)
    return b.getvalue()


if __name__ == '__main__':
    main()
