"""The C-ABI shared library loads on a CPU-only box and exports every symbol include/svc.h
declares; without a GPU svc_create reports an error instead of crashing."""
import ctypes
import os
import re
import struct

import pytest
import torch

from retargetvid_amd import _lib, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(svc_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    names = _declared()
    assert len(names) >= 10 and set(names) == set(_lib.EXPORTS)
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n


def test_struct_layout_matches_header():
    assert ctypes.sizeof(_lib.SvcParams) == 32
    assert [f[0] for f in _lib.SvcParams._fields_] == ['struct_size', 'hdbscan_min', 'hdbscan_min_samples', 'select_sum', 'op_close',
                                                       'clust_filt', 'resize_factor', 'com_km']


def test_abi_version_matches_header():
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    assert int(re.search(r'#define SVC_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == _lib.load().svc_abi_version()


def test_create_reports_errors():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.svc_create(b'\0' * 64, 64, 0, ctypes.byref(h)) < 0 and b'magic' in lib.svc_last_error()
    if not torch.cuda.is_available():
        blob = weights.pack_blob(weights.fold_state_dict(weights.make_synthetic_state_dict(0)))
        buf = ctypes.create_string_buffer(blob, len(blob))
        assert lib.svc_create(buf, len(blob), 0, ctypes.byref(h)) < 0
        assert len(lib.svc_last_error()) > 0
    assert lib.svc_destroy(None) == 0


def _blob_with_table(blob, table, magic=None, count=None):
    """The blob with another tensor table [(offset_floats, n_floats)] in front of the same payload (the offsets move with the header's
    size); magic / count: what the first two header words say instead of the blob's magic and len(table)."""
    m, nt = struct.unpack_from('<QQ', blob, 0)
    head = (16 + 16 * nt + 63) // 64 * 64
    new_head = (16 + 16 * len(table) + 63) // 64 * 64
    out = bytearray(new_head) + blob[head:]
    struct.pack_into('<QQ', out, 0, m if magic is None else magic, len(table) if count is None else count)
    for i, (off, n) in enumerate(table):
        struct.pack_into('<QQ', out, 16 + 16 * i, off + (new_head - head) // 4, n)
    return bytes(out)


@pytest.mark.gpu
def test_create_rejects_malformed_blobs(synthetic_sd):
    """svc_create names the blob's tensors in the order of weights.fold_state_dict: a blob with a tensor too few, one too many, a
    tensor of the wrong size, a wrong magic or a tensor count beyond its bytes is refused with SVC_E_BLOB and a message that says
    which; the blob as packed creates a handle.  No kernel is launched."""
    lib = _lib.load()
    layers = weights.fold_state_dict(synthetic_sd)
    blob = weights.pack_blob(layers)
    nt = struct.unpack_from('<QQ', blob, 0)[1]
    table = [struct.unpack_from('<QQ', blob, 16 + 16 * i) for i in range(nt)]
    assert _blob_with_table(blob, table) == blob
    names = [l['name'] for l in layers for _ in range(2 if 'b' in l else 1)]              # one per tensor: w, then b where there is one
    mid = names.index('skip_4x.reduce')                                                  # its weight: [64][128]
    assert table[mid][1] == 64 * 128
    wrong = list(table)
    wrong[mid] = (table[mid][0], table[mid][1] - 1)
    E_BLOB = -3
    cases = [('good', blob, 0, None),
             ('last tensor dropped', _blob_with_table(blob, table[:-1]), E_BLOB, b'blob: ran out of tensors at smoothing phase table'),
             ('one tensor appended', _blob_with_table(blob, table + [(table[0][0], 1)]), E_BLOB, b'1 unused tensors in blob'),
             ('wrong float count', _blob_with_table(blob, wrong), E_BLOB,
              b'blob: tensor %d (skip_4x.reduction) has 8191 floats, expected 8192' % mid),
             ('wrong magic', _blob_with_table(blob, table, magic=weights.BLOB_MAGIC + 1), E_BLOB, b'bad blob magic'),
             ('count past the bytes', _blob_with_table(blob, table, count=len(blob)), E_BLOB, b'truncated blob header')]
    for label, data, want, text in cases:
        h = ctypes.c_void_p()
        rc = lib.svc_create(ctypes.create_string_buffer(data, len(data)), len(data), 0, ctypes.byref(h))
        assert rc == want, (label, rc, lib.svc_last_error())
        if want:
            assert text in lib.svc_last_error() and not h.value, (label, lib.svc_last_error())
        else:
            assert h.value and lib.svc_destroy(h) == 0, label


def test_host_stage_entries_check_their_arguments():
    """The svc_host_* entries (host memory, no GPU): a SvcTemporalParams compiled against another layout is rejected by its
    struct_size, null / inconsistent arguments give SVC_E_INVALID + a message instead of a crash, n = 0 is a no-op."""
    import numpy as np
    lib = _lib.load()
    assert ctypes.sizeof(_lib.SvcTemporalParams) == 40
    assert [f[0] for f in _lib.SvcTemporalParams._fields_] == ['struct_size', 'lp_filt', 'lp_taps', 'loess_filt', 'loess_degree', 'reserved',
                                                               'loess_w_secs', 'fr']
    vp = ctypes.c_void_p
    xy = np.array([[10.0, 20.0], [11.0, 21.0], [12.0, 22.0]])
    cx, cy = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
    ti, seg, sel = np.array([0, 6, 11], np.int32), np.array([[0, 11]], np.int32), np.array([[0, 2]], np.int32)
    out = np.empty((4, 12))
    p = _lib.SvcTemporalParams(ctypes.sizeof(_lib.SvcTemporalParams), 0, 0, 1, 2, 0, 2.0, 30.0)
    args = lambda pp: (ctypes.byref(pp), None, None, None, cx.ctypes.data_as(vp), cy.ctypes.data_as(vp), 3, ti.ctypes.data_as(vp),
                       seg.ctypes.data_as(vp), sel.ctypes.data_as(vp), 1, 12, out[0].ctypes.data_as(vp), out[1].ctypes.data_as(vp),
                       out[2].ctypes.data_as(vp), out[3].ctypes.data_as(vp))
    assert lib.svc_host_temporal(*args(p)) == 12                          # 12 frames produced (linear interpolation of 3 samples)
    assert out[0][0] == 10.0 and out[0][6] == 11.0 and out[0][11] == 12.0
    stale = _lib.SvcTemporalParams(32, 0, 0, 1, 2, 0, 2.0, 30.0)          # a binding built against a shorter struct
    assert lib.svc_host_temporal(*args(stale)) == -1 and b'struct_size' in lib.svc_last_error()
    p_lp = _lib.SvcTemporalParams(ctypes.sizeof(_lib.SvcTemporalParams), 1, 6, 1, 2, 0, 2.0, 30.0)     # low-pass on, no coefficients
    assert lib.svc_host_temporal(*args(p_lp)) == -1
    assert lib.svc_host_loess(None, 0, 5, 2, None) == 0                   # n = 0: a no-op
    assert lib.svc_host_loess(None, 4, 5, 2, None) == -1
    assert lib.svc_host_boxes(None, None, 0, 640, 360, 250, 140, 120, 360, None, None, None, None) == 0
    assert lib.svc_host_interp_segment(None, None, None, 3, 3, None, None) == -1 and b'svc_host_interp_segment' in lib.svc_last_error()
    y = np.arange(8.0)
    o = np.empty(8)
    assert lib.svc_host_savgol(y.ctypes.data_as(vp), 8, 4, 2, o.ctypes.data_as(vp)) == -1          # even window: savgol_filter raises
    assert lib.svc_host_focus_stability(None, None, 0, None, 140, 250, 30.0, 6, 1.0, 60.0, 1.5, None, None) == 0
    assert lib.svc_host_focus_stability(None, None, 3, None, 140, 250, 30.0, 6, 1.0, 60.0, 1.5, None, None) == -1


def test_transnet_tap_door_constants_and_argument_checks():
    """svc_debug_transnet_tap (ABI 7): the layer ids of include/svc.h are the binding's, and a call without a handle is refused."""
    from retargetvid_amd import transnetv1_handler as Hd
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    ids = {k: int(v) for k, v in re.findall(r'#define SVC_SHOT_TAP_([A-Z0-9]+) (\d+)', text)}
    assert ids == {'INPUT': Hd.ShotTransNet.TAP_INPUT, 'CELL1': Hd.ShotTransNet.TAP_CELL1, 'POOL1': Hd.ShotTransNet.TAP_POOL1,
                   'DENSE': Hd.ShotTransNet.TAP_DENSE}
    assert len(Hd.ShotTransNet.TAP_SHAPES) == ids['DENSE'] + 1
    out = (ctypes.c_float * 4)()
    assert _lib.load().svc_debug_transnet_tap(None, None, 1, 4, 0, 4, 0, out, 4) == -1


def test_node_door_ids_are_the_headers_and_the_door_checks_its_arguments():
    """svc_debug_run_node: every SVC_NODE_* number of include/svc.h is ops.NODE_* and the tests' name table (net_node_cases.DEV_NODE),
    the two map nodes (26, 27; no ABI bump) included, and neither side has a name the other lacks; a call without a handle is refused."""
    from retargetvid_amd import ops
    import net_node_cases as C
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    ids = {k: int(v) for k, v in re.findall(r'#define SVC_NODE_([A-Z0-9_]+) (\d+)', text)}
    full = ids.pop('FULL')
    ids.update(F4X=full + 7, F2X=full + 14)
    assert re.search(r'#define SVC_NODE_F4X \(SVC_NODE_FULL \+ 7\)', text) and re.search(r'#define SVC_NODE_F2X \(SVC_NODE_FULL \+ 14\)', text)
    assert ids == {k[5:]: v for k, v in vars(ops).items() if k.startswith('NODE_')}
    assert (ids['MAP'], ids['MAP_PROFILE']) == (26, 27) == (ids['SMOOTH'] + 1, ids['SMOOTH'] + 2)
    named = {k.lower(): v for k, v in ids.items()}
    named.update({'block%d' % i: i for i in range(2, 18)})
    assert named == C.DEV_NODE
    for node in ('map', 'map_profile'):
        assert C.node_io(node, 256, 416, 140, 250) == ((32, 52), None, (2, 140, 250), None)
    out = (ctypes.c_float * 4)()
    lib = _lib.load()
    for node in (25, 26, 27, 28):
        assert lib.svc_debug_run_node(None, node, 1, 140, 250, ctypes.cast(out, ctypes.c_void_p), None, ctypes.cast(out, ctypes.c_void_p), 4) == -1
        assert b'svc_debug_run_node: invalid argument' in lib.svc_last_error()


def test_tail_plan_door_checks_its_arguments():
    """svc_debug_tail_plan (no ABI bump): without a handle, without an output or with too few words the call is refused with
    SVC_E_INVALID and a message, before anything is read."""
    from retargetvid_amd import ops
    from oracle import pipeline_ref as P
    lib = _lib.load()
    p = _lib.make_params(P.init_crop_params())
    n = len(ops.TAIL_PLAN_WORDS)
    out = (ctypes.c_int32 * n)()
    vp = ctypes.c_void_p
    assert lib.svc_debug_tail_plan(None, 140, 250, ctypes.byref(p), ctypes.cast(out, vp), n) == -1 and b'invalid argument' in lib.svc_last_error()
    assert lib.svc_debug_tail_plan(None, 140, 250, ctypes.byref(p), None, n) == -1 and b'svc_debug_tail_plan' in lib.svc_last_error()
    assert lib.svc_debug_tail_plan(None, 140, 250, ctypes.byref(p), ctypes.cast(out, vp), n - 1) == -1
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    assert int(re.search(r'#define SVC_TAILPLAN_WORDS (\d+)', text).group(1)) == n


def test_sort_plan_door_words_and_argument_checks():
    """svc_debug_sort_plan (no ABI bump; needs no handle and no GPU): every SVC_SORTPLAN_* of include/svc.h is a word of
    ops.SORT_PLAN_WORDS at the same index (case aside); n outside 1 .. 65 535, no output or too few words are refused with
    SVC_E_INVALID and a message; the entry came under revision 12 without a bump and is bound where the build has it."""
    from retargetvid_amd import ops
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    words = {k: int(v) for k, v in re.findall(r'#define SVC_SORTPLAN_([A-Z0-9_]+)\s+(\d+)', text)}
    n = words.pop('WORDS')
    assert n == len(ops.SORT_PLAN_WORDS) and words == {w.upper(): i for i, w in enumerate(ops.SORT_PLAN_WORDS)}
    history = text[:text.index('#define SVC_ABI_VERSION')]
    assert 'svc_debug_sort_plan' in history[history.index('(12, no bump)'):history.index(' * 13 = ')]
    assert 'svc_debug_sort_plan' in _lib.EXPORTS and 'svc_debug_sort_plan' in _lib.LATER_ENTRIES
    out = (ctypes.c_int32 * n)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    assert lib.svc_debug_sort_plan(1000, ptr, n) == n
    for args in ((0, ptr, n), (-1, ptr, n), (65536, ptr, n), (1000, None, n), (1000, ptr, n - 1)):
        assert lib.svc_debug_sort_plan(*args) == -1 and b'svc_debug_sort_plan' in lib.svc_last_error(), args
    for bad in (0, 65536):
        with pytest.raises(_lib.SvcError):
            ops.sort_plan(bad)
    for k in (1, 2, 3, 4, 1000, 32767, 32768, 65535):
        plan = ops.sort_plan(k)
        assert plan['depth'] == 2 * (k.bit_length() - 1) and plan['nseg'] == k // 17 + 2, k
        assert 0 < plan['lds_bytes'] and (plan['lds_bytes'] >= 16 * k) == bool(plan['in_lds']), k


def test_scratch_fill_door_takes_a_byte_or_off_and_nothing_else():
    """svc_debug_scratch_fill (ABI 13; needs no handle and no GPU): -1 and every byte are accepted, anything else is refused with
    SVC_E_INVALID and a message; ops.scratch_fill(None) is -1; the switch ends off."""
    from retargetvid_amd import ops
    lib = _lib.load()
    assert 'svc_debug_scratch_fill' in _lib.EXPORTS and 'svc_debug_scratch_fill' not in _lib.LATER_ENTRIES
    try:
        for byte in (0, 0x7F, 0xFF, -1):
            assert lib.svc_debug_scratch_fill(byte) == 0, byte
        for bad in (-2, 256, 1 << 20):
            assert lib.svc_debug_scratch_fill(bad) == -1 and b'svc_debug_scratch_fill' in lib.svc_last_error(), bad
            with pytest.raises(_lib.SvcError):
                ops.scratch_fill(bad)
        ops.scratch_fill(0xFF)
    finally:
        ops.scratch_fill(None)


def test_frame_header_words_are_the_headers():
    """The words of svc_debug_cluster_state's frame header: every SVC_HDR_* of include/svc.h is ops.HDR_* with the same number,
    neither side has a name the other lacks, and the named words and ranges lie side by side inside the header."""
    from retargetvid_amd import ops
    text = open(os.path.join(ROOT, 'include', 'svc.h')).read()
    words = {k: int(v) for k, v in re.findall(r'#define SVC_HDR_([A-Z0-9_]+)\s+(\d+)', text)}
    assert words == {k[4:]: v for k, v in vars(ops).items() if k.startswith('HDR_')} and len(words) == 25
    counts = {'CORE_STAMP0': 'CORE_STAMPS', 'LVL_PHASE0': 'LVL_PHASES', 'TP_STAMP0': 'TP_STAMPS'}      # first word of a range -> its count
    taken = []
    for k, v in words.items():
        if k != 'WORDS' and k not in counts.values():
            taken += range(v, v + (words[counts[k]] if k in counts else 1))
    assert sorted(taken) == list(range(31)) and words['WORDS'] == 32
