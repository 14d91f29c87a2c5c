"""Import the reference's smartVidCrop.py by path, in the BUILD CONTAINER ONLY, under stub modules for what it pulls in at import
time and the fixture generators never use (cv2, ffmpeg, hdbscan, imutils, tensorflow, the two network handlers, matplotlib ...).
A module that is installed is imported as it is; only a missing one is replaced by an empty module.  The reference's own LOESS
(3rd_party_libs/loess/pyloess.py) is found the way the reference finds it: its directory is put on sys.path first.

Shared by tools/make_golden_border.py, tools/make_golden_refpath.py and tools/make_golden_refpath_clustered.py.  Nothing at test, bench or smoke time imports this file."""
import contextlib
import importlib.util
import io
import os
import sys
import types


class _Any:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Any()

    def __getattr__(self, n):
        return _Any()


def load_reference(ref_dir):
    loess_dir = os.path.join(os.path.abspath(ref_dir), '3rd_party_libs', 'loess')      # (smartVidCrop.py:80-83)
    if os.path.isdir(loess_dir) and loess_dir not in sys.path:
        sys.path.insert(0, loess_dir)
    for name in ('cv2', 'ffmpeg', 'hdbscan', 'imutils', 'imutils.video', 'tensorflow', 'transnetv1_handler', 'unisal_handler',
                 'matplotlib', 'matplotlib.pyplot', 'sklearn', 'sklearn.cluster', 'scipy', 'scipy.signal', 'scipy.interpolate',
                 'pyloess'):
        if name in sys.modules:
            continue
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    cv2 = sys.modules['cv2']
    if not hasattr(cv2, 'getTickCount'):
        cv2.getTickCount, cv2.getTickFrequency = (lambda: 0), (lambda: 1.0)
    tf = sys.modules['tensorflow']
    if not hasattr(tf, 'Session'):
        tf.GPUOptions = tf.Session = tf.ConfigProto = _Any
    th = sys.modules['transnetv1_handler']
    th.ShotTransNetParams = th.ShotTransNet = _Any
    sys.modules['unisal_handler'].init_unisal_for_images = lambda: None
    iv = sys.modules['imutils.video']
    if not hasattr(iv, 'FileVideoStream'):
        iv.FileVideoStream = iv.FPS = object
    spec = importlib.util.spec_from_file_location('ref_svc', os.path.join(ref_dir, 'smartVidCrop.py'))
    m = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(m)
    return m
