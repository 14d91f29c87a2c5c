"""The network plan's geometry (svc_debug_net_plan: host arithmetic of the library, no GPU) over EVERY map shape the ingest can
hand the network, against the oracle's restatement of it.

Three kernels of the network do work that depends on the map shape (h, w) itself, not only on the network size it selects:
k_front and k_lanczos_norm (Pillow LANCZOS (h, w) -> (NH, NW)) and k_smooth_down_mfma (smoothing + bilinear (NH, NW) -> (h, w)).
The census: the ingest's shapes -- oracle.pipeline_ref.sal_size(W, H, 250) for sources of 64..4096 px -- and the square
8..255 x 8..255 that the ABI accepts and the tail can cluster.  Asserted for every shape: it selects one of the eleven network
sizes and runs the fused front kernel; the dynamic LDS of all three kernels is within what their launcher allows; NH, NW and the
tables' tap counts are the oracle's, and k_front's source window (rows / columns one tile needs at most), restated here on
oracle.lanczos_ref.precompute_coeffs's bounds, is the door's; the rows per band of k_smooth_down_mfma are the most whose band
fits (restated here in float32).  And SHAPES, the table tests/test_gpu_map_shapes.py runs on the device, attains the extremes
of the census: a change of FR_TH / FR_TW / SD_ROWS or of a budget moves an extreme, and this file names the shape that shows it."""
import functools

import numpy as np
import pytest

from oracle import lanczos_ref, pipeline_ref as P, unisal_ref as U
from retargetvid_amd import ops
from test_oracle_unisal import NET_SIZES

# ---- the table of tests/test_gpu_map_shapes.py: (h, w) -> why it is there ---------------------------------------------------
SHAPES = {
    # realistic ratios outside the eleven of test_oracle_unisal.ELEVEN
    (104, 250): '2.39:1', (250, 104): '1:2.39', (90, 250): '2.76:1', (125, 250): '2:1', (156, 250): '16:10', (113, 250): '2.2:1',
    (241, 249): 'fr_nr at its maximum (22) on a non-square map',
    (240, 251): 'fr_nc = 35, the maximum of the square, reached through the ABI only',
    # narrow: few source columns per tile of k_front
    (250, 70): 'narrow 9:32', (250, 35): 'narrow', (250, 20): 'narrow', (250, 8): 'fr_nc at its minimum (7)',
    # wide, down to strips: many network rows per map row in k_smooth_down_mfma
    (70, 250): '32:9, 7 rows per band', (64, 250): 'the lowest h x 250 with 7 rows per band', (63, 250): 'the first with fewer (6)',
    (48, 250): '5 rows per band', (35, 250): '4 rows per band', (27, 250): '3 rows per band', (20, 250): '2 rows per band',
    (19, 250): 'the lowest map that fitted the CU with 7 rows per band (159 104 B)', (18, 250): 'the first that did not (165 760 B)',
    (12, 250): 'strip', (8, 250): 'fr_nr at its minimum (7), 1 row per band, sd_tile_cap at its minimum (2)',
    (8, 8): 'smallest both ways',
    (31, 8): 'sd_tile_cap at its maximum (43): 4 map rows over 416 network rows of 256',
    # an axis that is not resampled (in_size == out_size: lanczos_tab's one-tap table); saliency entry only (the tail takes <= 255)
    (416, 256): 'identity on both axes', (416, 250): 'identity on the rows',
}
# down-scaling frames: eleven-tap tables and more, the three-kernel path.  540x960: the largest k_lanczos_norm tile that fits.
DOWN_SHAPES = {(360, 640): 81568, (480, 640): None, (417, 257): None, (540, 960): 143616}
REFUSED = {(720, 1280): 226272, (1080, 1920): 436768}

# ---- the constants of csrc/svc_net.hip, restated ------------------------------------------------------------------------------
FR_TH, FR_TW = 8, 16
FR_PR, FR_PC = 2 * (FR_TH + 2) + 1, 2 * (FR_TW + 2) + 1
FR_SONLY_BYTES = (FR_TH + 2) * (FR_TW + 2) * 36 * 4
FR_IN_BYTES = FR_PR * 112 * 4
SD_ROWS, SD_KP = 7, 56
KB64, KB160 = 64 * 1024, 160 * 1024


@functools.lru_cache(maxsize=None)
def ingest_shapes():
    out = set()
    for W in range(64, 4097, 2):
        for H in range(64, 4097, 8):
            h, w = P.sal_size(W, H, 250)
            if h >= 8 and w >= 8:
                out.add((h, w))
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def census():
    """{(h, w): the door's words} over the ingest's shapes and the square 8..255 x 8..255."""
    shapes = ingest_shapes() | {(h, w) for h in range(8, 256) for w in range(8, 256)}
    return {s: ops.net_plan(*s) for s in sorted(shapes)}


@functools.lru_cache(maxsize=None)
def axis_tables(in_size, out_size):
    """(bounds [out, 2], taps) of one axis: the oracle's; an axis of equal sizes is not resampled (Pillow skips the pass), which
    the library states as a one-tap table."""
    if in_size == out_size:
        return np.stack([np.arange(out_size), np.ones(out_size, int)], 1), 1
    bounds, _, ksize = lanczos_ref.precompute_coeffs(in_size, out_size)
    return bounds.astype(int), ksize


def front_window(bounds, N, T, PR):
    """Source rows (columns) a tile of T stem rows needs at most: the patch of PR input rows from 2 t T - 3, clipped to the image."""
    n = 0
    for t in range(-(-(N // 2) // T)):
        a, b = max(2 * t * T - 3, 0), min(2 * t * T - 3 + PR, N)
        n = max(n, bounds[b - 1][0] + bounds[b - 1][1] - bounds[a][0])
    return int(n)


def front_ok(vb, vks, hks, nr, nc):
    stride = ((nc * 3 + 6) >> 2) << 2
    small = ((nr * (stride + 112) + 15) & ~15) + 768 * 4
    return bool(hks <= 7 and vks <= 7 and (np.diff(vb[:, 0]) <= 1).all() and nr <= 32 and stride <= 128 and small <= FR_SONLY_BYTES)


def sd_band(h, NH, rows):
    """Network-size rows a band of `rows` map rows needs at most: the kernel's float32 arithmetic."""
    f = np.float32
    scy = f(NH) / f(h)
    oy0 = np.arange(0, h, rows)
    oy1 = np.minimum(h, oy0 + rows)
    ylo = np.maximum(scy * (oy0.astype(f) + f(0.5)) - f(0.5), f(0)).astype(int)
    yhi = np.minimum(np.maximum(scy * ((oy1 - 1).astype(f) + f(0.5)) - f(0.5), f(0)).astype(int) + 1, NH - 1)
    return int((yhi - ylo + 1).max())


def sd_lds(NH, NW, cap):
    return ((NH // 8) * (NW // 8) + 64 * SD_KP + cap * NW) * 4


def test_the_census_is_the_ingests_968_shapes_and_the_square():
    ing = ingest_shapes()
    assert len(ing) == 968 and all(max(s) in (249, 250) for s in ing), len(ing)
    assert min(h for h, _ in ing) == 8 and min(w for _, w in ing) == 8
    assert len(census()) == len(ing | {(h, w) for h in range(8, 256) for w in range(8, 256)})


def test_every_shape_selects_one_of_the_eleven_sizes_and_runs_the_fused_front():
    sizes = set(NET_SIZES.values())
    for (h, w), p in census().items():
        assert (p['NH'], p['NW']) in sizes, ((h, w), p)
        assert p['fr_ok'] == 1, ((h, w), 'the shape would run the three kernels', p)
        assert (p['fr_tiles_y'], p['fr_tiles_x']) == (-(-(p['NH'] // 2) // FR_TH), -(-(p['NW'] // 2) // FR_TW)), ((h, w), p)


def test_every_lds_request_is_within_what_its_launcher_allows():
    for (h, w), p in census().items():
        assert (p['lz_lds_max'], p['sd_lds_max'], p['fr_lds_max']) == (KB160, KB64, KB64)
        assert p['fr_lds'] == FR_IN_BYTES + FR_SONLY_BYTES <= p['fr_lds_max'], ((h, w), p)
        assert 0 < p['lz_lds'] <= p['lz_lds_max'], ((h, w), 'k_lanczos_norm', p['lz_lds'])
        assert 0 < p['sd_lds'] <= p['sd_lds_max'], ((h, w), 'k_smooth_down_mfma', p['sd_lds'], p['sd_rows'])
        assert p['sd_lds'] == sd_lds(p['NH'], p['NW'], p['sd_tile_cap']), ((h, w), p)


def _against_the_oracle(h, w, p):
    assert (p['NH'], p['NW']) == U.get_optimal_out_size((h, w)), ((h, w), p)
    vb, vks = axis_tables(h, p['NH'])
    hb, hks = axis_tables(w, p['NW'])
    assert (p['vks'], p['hks']) == (vks, hks), ((h, w), p)
    nr, nc = front_window(vb, p['NH'], FR_TH, FR_PR), front_window(hb, p['NW'], FR_TW, FR_PC)
    ok = front_ok(vb, vks, hks, nr, nc)
    assert p['fr_ok'] == ok, ((h, w), p, nr, nc)
    if ok:
        assert (p['fr_nr'], p['fr_nc']) == (nr, nc), ((h, w), p, nr, nc)
    y1 = np.minimum(np.arange(0, p['NH'], 8) + 8, p['NH']) - 1
    cap = int((vb[y1, 0] + vb[y1, 1] - vb[::8, 0]).max())                    # k_lanczos_norm: bands of 8 network rows
    assert p['lz_tile_cap'] == cap, ((h, w), p, cap)
    r16 = lambda v: (v + 15) // 16 * 16
    assert p['lz_lds'] == r16(cap * w * 3) + r16(cap * p['NW'] * 3) + p['NW'] * hks * 4 + 768 * 4, ((h, w), p)


def test_the_door_agrees_with_the_oracle_at_every_shape():
    for (h, w), p in census().items():
        _against_the_oracle(h, w, p)


def test_the_rows_per_band_are_the_most_whose_band_fits():
    """Every shape of the ingest, every shape of the square that does not keep SD_ROWS rows, and every 16th other."""
    ing = ingest_shapes()
    for i, ((h, w), p) in enumerate(census().items()):
        if (h, w) not in ing and p['sd_rows'] == SD_ROWS and i % 16:
            continue
        r = p['sd_rows']
        assert 1 <= r <= SD_ROWS and p['sd_tile_cap'] == sd_band(h, p['NH'], r), ((h, w), p)
        if r < SD_ROWS:
            assert sd_lds(p['NH'], p['NW'], sd_band(h, p['NH'], r + 1)) > KB64, ((h, w), 'a band of %d rows fits too' % (r + 1), p)


def test_the_table_of_the_device_tests_attains_the_extremes_of_the_census():
    c = census()
    table = {s: ops.net_plan(*s) for s in SHAPES}
    for s, p in table.items():
        _against_the_oracle(s[0], s[1], p)
        assert p['fr_ok'] == 1 and p['sd_lds'] <= KB64 and p['lz_lds'] <= KB160, (s, p)
    in_census = {s: p for s, p in table.items() if s in c}
    assert set(table) - set(in_census) == {(416, 256), (416, 250)}
    assert table[(416, 256)]['hks'] == table[(416, 256)]['vks'] == table[(416, 250)]['vks'] == 1 and table[(416, 250)]['hks'] == 7
    for key in ('fr_nr', 'fr_nc', 'sd_tile_cap'):
        lo, hi = min(p[key] for p in c.values()), max(p[key] for p in c.values())
        have = {p[key] for p in in_census.values()}
        assert lo in have and hi in have, (key, lo, hi, [s for s, p in c.items() if p[key] in (lo, hi)][:6])
    assert (min(p['fr_nr'] for p in c.values()), max(p['fr_nr'] for p in c.values())) == (7, 22)
    assert (min(p['fr_nc'] for p in c.values()), max(p['fr_nc'] for p in c.values())) == (7, 35)
    assert max(p['fr_nc'] for s, p in c.items() if s in ingest_shapes()) == 34
    assert table[(241, 249)]['fr_nr'] == 22 and table[(240, 251)]['fr_nc'] == 35
    # every number of rows per band the plan chooses, and both sides of the threshold below which it chooses fewer than SD_ROWS
    rows = {p['sd_rows'] for p in c.values()}
    assert rows == set(range(1, SD_ROWS + 1)) == {p['sd_rows'] for p in in_census.values()}, rows
    strips = {h: c[(h, 250)]['sd_rows'] for h in range(8, 251)}
    first = max(h for h, r in strips.items() if r < SD_ROWS)
    assert all(r == SD_ROWS for h, r in strips.items() if h > first) and (first, first + 1) == (63, 64)
    assert (first, 250) in SHAPES and (first + 1, 250) in SHAPES
    # ... and of the CU's 160 KB, which the strips met with SD_ROWS rows per band whatever their LDS came to
    old = {h: sd_lds(256, 416, sd_band(h, 256, SD_ROWS)) for h in range(8, 64)}
    assert (old[19], old[18]) == (159104, 165760) and max(h for h in old if old[h] > KB160) == 18 and max(old.values()) == old[8] == 343808


def test_the_down_scaling_frames_and_the_refused_ones():
    for s, lds in list(DOWN_SHAPES.items()) + list(REFUSED.items()):
        p = ops.net_plan(*s)
        _against_the_oracle(s[0], s[1], p)
        assert p['fr_ok'] == 0 and (lds is None or p['lz_lds'] == lds), (s, p)
        assert (p['lz_lds'] <= KB160) == (s in DOWN_SHAPES), (s, p)
    p = ops.net_plan(417, 257)
    assert (p['NH'], p['NW'], p['vks'], p['hks']) == (416, 256, 9, 9)             # out of k_front by one pixel either way


def test_the_door_refuses_invalid_arguments():
    import ctypes
    from retargetvid_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 32)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    assert lib.svc_debug_net_plan(140, 250, ptr, 32) == len(ops.PLAN_WORDS)
    for args in ((7, 250, ptr, 32), (140, 7, ptr, 32), (140, 250, None, 32), (140, 250, ptr, len(ops.PLAN_WORDS) - 1)):
        assert lib.svc_debug_net_plan(*args) == -1 and b'svc_debug_net_plan' in lib.svc_last_error(), args
    with pytest.raises(_lib.SvcError):
        ops.net_plan(4, 250)
