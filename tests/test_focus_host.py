"""svc_host_focus_hold (csrc/svc_host.cpp; temporal.focus_hold_native): the second half of the focus stability on its own -- the
list of low-saliency jumps and the hold loop (smartVidCrop.py:2448-2473) -- from jump statistics it is GIVEN.  The device route
(svc_focus_jumps_u8, tests/test_gpu_focus.py) hands it the statistics the kernel computed; here it is fed the oracle's own list
(oracle/temporal_ref.focus_stability) and must return the oracle's held centres and indices, exactly.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import focus_cases as F
from oracle import pipeline_ref as P, temporal_ref as TR
from retargetvid_amd import _lib, temporal

SHAPES = F.SHAPES[:2]               # 35 x 62 and 140 x 250


def test_the_hold_from_the_oracles_jumps_is_the_oracles_hold():
    rng = np.random.RandomState(0)
    n_inds = n_held = 0
    for trial in range(32):
        n = rng.randint(7, 40)
        h, w = SHAPES[(trial // 4) % 2]
        maps = F.random_maps(rng, n, h, w)
        dx, dy = F.centres(rng, trial % 4, n, h, w)
        hwn = np.ascontiguousarray(np.transpose(maps, (1, 2, 0)))
        for best in (True, False):
            CP = dict(P.init_crop_params(best), foces_stab_t=int(rng.choice([60, 120, 200])))
            rx, ry, rj, ri = TR.focus_stability(list(dx), list(dy), hwn, 30.0, CP)
            xy, inds = temporal.focus_hold_native(np.stack([dx, dy], 1), rj, 30.0, CP)
            assert inds == list(ri) and xy[:, 0].tolist() == list(rx) and xy[:, 1].tolist() == list(ry), (trial, best)
            n_inds += len(inds)
            n_held += int((xy[:, 0] != np.array(dx)).sum())
    assert n_inds > 100 and n_held > 20            # the loop had jumps to list and centres to hold


def test_the_hold_of_no_frame_and_of_one_frame():
    CP = P.init_crop_params(True)
    xy, inds = temporal.focus_hold_native(np.zeros((0, 2)), [], 30.0, CP)
    assert xy.shape == (0, 2) and inds == []
    xy, inds = temporal.focus_hold_native(np.array([[3.5, 4.25]]), [0.0], 30.0, CP)       # frame 0 is never listed, whatever its jump
    assert xy.tolist() == [[3.5, 4.25]] and inds == []
    with pytest.raises(ValueError):
        temporal.focus_hold_native(np.zeros((3, 2)), [255, 255], 30.0, CP)


def test_the_hold_entry_checks_its_arguments():
    lib = _lib.load()
    assert 'svc_host_focus_hold' in _lib.EXPORTS and 'svc_host_focus_hold' in _lib.LATER_ENTRIES
    vp = ctypes.c_void_p
    cx, cy, j = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0]), np.array([255.0, 10.0, 10.0])
    inds = np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data_as(vp)
    assert lib.svc_host_focus_hold(None, None, 0, None, 30.0, 6, 60.0, 1.5, None) == 0                       # n = 0: a no-op
    assert lib.svc_host_focus_hold(p(cx), p(cy), 3, p(j), 30.0, 6, 60.0, 1.5, p(inds)) == 2 and inds.tolist()[:2] == [1, 2]
    assert cx.tolist() == [1.0, 1.0, 3.0]          # (start 0, end 2, 12 frames at 30 fps <= 1.5 s: centres 0 and 1 take centre 0)
    for args in ((None, p(cy), 3, p(j), 30.0, 6, 60.0, 1.5, p(inds)), (p(cx), None, 3, p(j), 30.0, 6, 60.0, 1.5, p(inds)),
                 (p(cx), p(cy), 3, None, 30.0, 6, 60.0, 1.5, p(inds)), (p(cx), p(cy), 3, p(j), 30.0, 6, 60.0, 1.5, None),
                 (p(cx), p(cy), -1, p(j), 30.0, 6, 60.0, 1.5, p(inds)), (p(cx), p(cy), 3, p(j), 0.0, 6, 60.0, 1.5, p(inds)),
                 (p(cx), p(cy), 3, p(j), float('nan'), 6, 60.0, 1.5, p(inds))):
        assert lib.svc_host_focus_hold(*args) == -1 and b'svc_host_focus_hold' in lib.svc_last_error(), args


def test_the_device_entry_checks_its_arguments_before_it_touches_the_device():
    """svc_focus_jumps_u8 (no handle): n = 0 is a no-op and a bad argument is SVC_E_INVALID with a message, both without a GPU --
    the entry decides before its launch.  (Pointers here are never dereferenced on the host.)"""
    lib = _lib.load()
    assert 'svc_focus_jumps_u8' in _lib.EXPORTS and 'svc_focus_jumps_u8' in _lib.LATER_ENTRIES
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'svc.h')).read()
    history = text[:text.index('#define SVC_ABI_VERSION')]
    for name in ('svc_focus_jumps_u8', 'svc_host_focus_hold'):
        assert name in history[history.index('(12, no bump)'):history.index(' * 13 = ')]
    assert '#define SVC_FOCUS_MAX_COORD 65536\n' in text
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.svc_focus_jumps_u8(None, 0, 35, 62, None, 1.0, None, None) == 0
    for args in ((ptr, -1, 35, 62, ptr, 1.0, ptr, None), (ptr, 0, 0, 62, ptr, 1.0, ptr, None), (ptr, 0, 35, 0, ptr, 1.0, ptr, None),
                 (ptr, 0, 35, 62, ptr, float('nan'), ptr, None), (None, 2, 35, 62, ptr, 1.0, ptr, None), (ptr, 2, 35, 62, None, 1.0, ptr, None),
                 (ptr, 2, 35, 62, ptr, 1.0, None, None), (ptr, 2, 35, 62, ptr, 1.0, ctypes.c_void_p(buf.ctypes.data + 4), None)):
        assert lib.svc_focus_jumps_u8(*args) == -1 and b'svc_focus_jumps_u8' in lib.svc_last_error(), args
