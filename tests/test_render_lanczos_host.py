"""The renderer's Lanczos filter without a GPU: the new entry in header and binding, its argument checks, the interp= doors that
refuse an unknown filter before any device work, and the table builder (csrc/svc_lanczos.h) compiled on its own against
oracle/lanczos_ref.precompute_coeffs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import lanczos_ref
from retargetvid_amd import _lib, ops, render, smartVidCrop as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'svc.h')).read()


def test_header_binding_and_abi_version_agree():
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    proto = re.search(r'int\s+svc_render_crops_filter\s*\(([^)]*)\)\s*;', text)
    assert proto, 'svc_render_crops_filter is not declared'
    params = [' '.join(p.split()) for p in proto.group(1).split(',')]
    assert params == ['SvcHandle *h', 'const uint8_t *frames', 'const SvcFrameLayout *layout', 'int n', 'int height', 'int width',
                      'const int32_t *boxes', 'int bw', 'int bh', 'uint8_t *out', 'int out_fmt', 'int oh', 'int ow',
                      'int filter', 'int flags', 'void *stream']
    assert 'svc_render_crops_filter' in _lib.EXPORTS
    lib = _lib.load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = [i32 if p.startswith('int ') else ctypes.POINTER(_lib.SvcFrameLayout) if 'SvcFrameLayout' in p else vp for p in params]
    assert lib.svc_render_crops_filter.argtypes == want and lib.svc_render_crops_filter.restype == i32
    ids = {k: int(v) for k, v in re.findall(r'#define SVC_FILTER_([A-Z]+)\s+(\d+)', text)}
    assert ids == {'LINEAR': _lib.FILTER_LINEAR, 'LANCZOS': _lib.FILTER_LANCZOS}
    assert [ids[k.upper()] for k in ops.INTERPS] == [0, 1] and ops.INTERPS == ('linear', 'lanczos')
    assert int(re.search(r'#define SVC_ABI_VERSION (\d+)', text).group(1)) == 13 == _lib.ABI_VERSION == lib.svc_abi_version()


def test_entry_checks_its_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(16)                   # never dereferenced: every call below fails validation first
    rgb = ops.frame_layout('rgb24', 360, 640).struct()
    ok = dict(h=fake, frames=fake, layout=rgb, n=2, height=360, width=640, boxes=fake, bw=120, bh=360, out=fake, out_fmt=0,
              oh=720, ow=240, filter=_lib.FILTER_LANCZOS, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.svc_render_crops_filter(a['h'], a['frames'], ctypes.byref(a['layout']), a['n'], a['height'], a['width'], a['boxes'],
                                         a['bw'], a['bh'], a['out'], a['out_fmt'], a['oh'], a['ow'], a['filter'], a['flags'], None)
        return rc, lib.svc_last_error().decode()

    for bad, rule in ((dict(filter=2), 'svc_render_crops_filter: unknown filter 2'),
                      (dict(filter=-1), 'svc_render_crops_filter: unknown filter -1'),
                      (dict(out_fmt=2), 'svc_render_crops_filter: unknown out_fmt 2'),
                      (dict(out_fmt=1, flags=ops.RENDER_BGR), 'flags must be 0 (SVC_RENDER_BGR has no meaning for an NV12 output)'),
                      (dict(out_fmt=1, oh=721), 'width and height of an NV12 output are even and >= 2'),
                      (dict(out_fmt=1, ow=241), 'width and height of an NV12 output are even and >= 2'),
                      (dict(bw=641), 'svc_render_crops_filter: invalid argument'),
                      (dict(bh=361), 'svc_render_crops_filter: invalid argument'),
                      (dict(flags=2), 'flags has bits other than SVC_RENDER_BGR'),
                      (dict(h=None), 'svc_render_crops_filter: invalid argument'),
                      (dict(frames=None), 'svc_render_crops_filter: invalid argument'),
                      (dict(oh=0), 'an RGB output has width and height >= 1')):
        rc, msg = call(**bad)
        assert rc == -1 and rule in msg, (bad, rc, msg)
    # the linear filter is the existing entry: its checks, under its name
    rc, msg = call(filter=_lib.FILTER_LINEAR, bw=641)
    assert rc == -1 and msg.startswith('svc_render_crops_layout: invalid argument')
    rc, msg = call(filter=_lib.FILTER_LINEAR, flags=2)
    assert rc == -1 and msg.startswith('svc_render_crops_layout: ') and 'SVC_RENDER_BGR' in msg
    # the layout rules are the existing ones
    stale = ops.frame_layout('rgb24', 360, 640).struct()
    stale.struct_size = 32
    rc, msg = call(layout=stale)
    assert rc == -1 and 'struct_size is 32' in msg


def test_python_doors_refuse_an_unknown_interp_before_device_work():
    frames = np.zeros((3, 36, 64, 3), np.uint8)
    boxes = np.array([[0, 0, 10, 36]] * 3, np.int32)
    with pytest.raises(ValueError, match='cubic'):
        ops.Engine.render_crops(None, frames, boxes, out_hw=(72, 20), interp='cubic')      # (no engine: nothing reaches one)
    with pytest.raises(ValueError, match='cubic'):
        render.render_video(frames, dict(fc=3, bbs_np=boxes.astype(np.int64)), engine=None, out_size=(20, 72), interp='cubic')
    video = dict(fr=30.0, frame_count=3, w=64, h=36, frames=frames, trans_inds=[0, 3])
    with pytest.raises(ValueError, match='cubic'):
        S.smart_vid_crop(video, out_size=(20, 72), out_interp='cubic')
    assert ops.check_interp('linear') == 'linear' and ops.check_interp('lanczos') == 'lanczos'


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('native') / 'liblanczos_tab_harness.so')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', out,
                           os.path.join(ROOT, 'tests', 'native', 'lanczos_tab_harness.cpp')])
    lib = ctypes.CDLL(out)
    lib.lanczos_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return lib


def _dense(bounds, coef, in_size):
    """The table as the [out][in] matrix it applies."""
    m = np.zeros((len(bounds), in_size), np.int64)
    for i, (lo, cnt) in enumerate(bounds):
        m[i, lo:lo + cnt] = coef[i, :cnt]
    return m


@pytest.mark.parametrize('sizes', [(607, 1080), (1215, 720), (5, 7), (640, 36), (77, 77)])
def test_table_builder_stands_alone_and_equals_the_oracle(harness, sizes):
    """Equal sizes: Pillow skips the pass, lanczos_tab gives the identity table (one tap of 1 << 22) and precompute_coeffs the same
    filter with the zero taps around it spelled out -- compared as the matrices they apply, like every other pair; the pairs
    that resample are compared entry by entry as well."""
    n_in, n_out = sizes
    rb, rc, rks = lanczos_ref.precompute_coeffs(n_in, n_out)
    cap = n_out * max(rks, 1)
    bounds, coef = np.full((n_out, 2), -1, np.int32), np.full(cap, -1, np.int32)
    ks = harness.lanczos_table(n_in, n_out, bounds.ctypes.data, bounds.size, coef.ctypes.data, coef.size)
    assert 1 <= ks <= rks
    coef = coef[:n_out * ks].reshape(n_out, ks)
    assert (bounds >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ks).all()
    assert np.array_equal(_dense(bounds, coef, n_in), _dense(rb, rc, n_in))
    if n_in != n_out:
        assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coef, rc)
        # what the launcher asserts before it uses a table: exact 24-bit products, Pillow's int32 range
        assert np.abs(coef).max() < 1 << 23 and 255 * int(np.abs(coef.astype(np.int64)).sum(1).max()) + (1 << 21) < 1 << 31
    else:
        assert ks == 1 and np.array_equal(bounds, np.stack([np.arange(n_out), np.ones(n_out, int)], 1)) and (coef == 1 << 22).all()
