"""The five-panel demo frames restated in NumPy, and the cases of the demo tests (a helper module, not a conftest).

compose() is written from the rules include/svc.h states for svc_demo_frames_u8, not from the kernel: panels first, then the
marks of every frame in list order, each confined to its own panel.  Everything is int64 on whole panel grids.  The one place
that needs a word: the inner test of a LINE, 4 (e x d)^2 <= p^2 L, is evaluated as (e x d)^2 <= (p^2 L) // 4 where |e x d| < 2^31
and as False elsewhere -- for integers 4 c^2 <= M is c^2 <= floor(M / 4), and M = p^2 L <= 255^2 * 2 * 65534^2 < 2^50 < 4 * 2^62, so
this is the same statement without an int64 overflow.

The mark words: {kind | panel << 8, x0, y0, x1, y1, p, q, r | g << 8 | b << 16}."""
import numpy as np

DISC, LINE, RECT, TEXT = 0, 1, 2, 3
WORDS, MAX_MARKS, PANELS = 8, 64, 5
COORD, SPRITE = 32767, 4096


def mean_even(a, b):
    """(a + b) / 2 with ties to even, in integers: s = a + b; v = s >> 1; v += s & v & 1."""
    s = a.astype(np.int64) + b.astype(np.int64)
    v = s >> 1
    return v + (s & v & 1)


def mark(kind, panel, x0=0, y0=0, x1=0, y1=0, p=0, q=0, rgb=(255, 255, 255)):
    return [kind | panel << 8, x0, y0, x1, y1, p, q, rgb[0] | rgb[1] << 8 | rgb[2] << 16]


def _ignored(w):
    kind, panel = w[0] & 0xff, w[0] >> 8
    if w[0] < 0 or kind > TEXT or panel >= PANELS or any(abs(int(v)) > COORD for v in w[1:5]):
        return True
    if kind in (DISC, LINE):
        return not 0 <= w[5] <= 255
    if kind == TEXT:
        return w[6] < 0 or (w[6] & 0xffff) > SPRITE or (w[6] >> 16) > SPRITE
    return False


def coverage(w, ph, pw, atlas):
    """One mark on its ph x pw panel -> (covered bool [ph, pw], coverage int64 [ph, pw]); an ignored mark covers nothing."""
    w = [int(v) for v in w]
    none = np.zeros((ph, pw), bool)
    a = np.full((ph, pw), 255, np.int64)
    if _ignored(w):
        return none, a
    kind, x0, y0, x1, y1, p, q = w[0] & 0xff, w[1], w[2], w[3], w[4], w[5], w[6]
    y, x = np.meshgrid(np.arange(ph, dtype=np.int64), np.arange(pw, dtype=np.int64), indexing='ij')
    if kind == DISC:
        return (x - x0) ** 2 + (y - y0) ** 2 <= p * p, a
    if kind == LINE:
        dx, dy, ex, ey = x1 - x0, y1 - y0, x - x0, y - y0
        L, u = dx * dx + dy * dy, ex * dx + ey * dy
        near0 = 4 * (ex * ex + ey * ey) <= p * p
        near1 = 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= p * p
        c = np.abs(ex * dy - ey * dx)
        small = c < 2 ** 31
        inner = small & (np.where(small, c, 0) ** 2 <= (p * p * L) // 4)
        if L == 0:
            return near0, a
        return np.where(u <= 0, near0, np.where(u >= L, near1, inner)), a
    if kind == RECT:
        inside = (x0 <= x) & (x <= x1) & (y0 <= y) & (y <= y1)
        return inside & ((x == x0) | (x == x1) | (y == y0) | (y == y1)), a
    sw, sh = q & 0xffff, q >> 16
    inside = (0 <= x - x0) & (x - x0 < sw) & (0 <= y - y0) & (y - y0 < sh)
    at = p + (y - y0) * sw + (x - x0)
    n_atlas = 0 if atlas is None else len(atlas)
    ok = inside & (at >= 0) & (at < n_atlas)
    if n_atlas:
        a = np.where(ok, np.asarray(atlas, np.int64)[np.clip(at, 0, n_atlas - 1)], 255)
    return ok, a


def compose(small, raw, filt, map_of, marks, first, atlas, bgr=False):
    """small uint8 [n, ph, pw, 3], raw / filt uint8 [n_maps, ph, pw], map_of [n], marks [k, 8], first [n + 1], atlas uint8 [bytes] or
    None -> uint8 [n, ph, 5 * pw, 3]."""
    small = np.asarray(small)
    n, ph, pw, _ = small.shape
    n_maps, k = len(raw), len(marks)
    marks = np.asarray(marks, np.int64).reshape(-1, WORDS)
    out = np.empty((n, ph, PANELS * pw, 3), np.uint8)
    zero = np.zeros((ph, pw), np.int64)
    for f in range(n):
        S = small[f].astype(np.int64)
        m = int(map_of[f])
        r, g = (raw[m].astype(np.int64), filt[m].astype(np.int64)) if 0 <= m < n_maps else (zero, zero)
        rep = lambda v: np.repeat(v[:, :, None], 3, axis=2)
        panels = [S.copy(), rep(r), rep(g), mean_even(S, rep(g)), S.copy()]
        lo, hi = (min(max(int(v), 0), k) for v in (first[f], first[f + 1]))
        for w in marks[lo:lo + min(max(hi - lo, 0), MAX_MARKS)]:
            panel = int(w[0]) >> 8
            cov, a = coverage(w, ph, pw, atlas)
            if not cov.any():
                continue
            P = panels[panel]
            for c in range(3):
                colour = (int(w[7]) >> (8 * c)) & 255
                P[:, :, c] = np.where(cov, (colour * a + P[:, :, c] * (255 - a) + 127) // 255, P[:, :, c])
        frame = np.concatenate(panels, axis=1)
        out[f] = frame[:, :, ::-1] if bgr else frame
    return out


# ---- case builders ----------------------------------------------------------------------------------------------------

def inputs(n, ph, pw, n_maps, seed):
    rng = np.random.RandomState(seed)
    small = rng.randint(0, 256, (n, ph, pw, 3)).astype(np.uint8)
    raw = rng.randint(0, 256, (n_maps, ph, pw)).astype(np.uint8)
    filt = rng.randint(0, 256, (n_maps, ph, pw)).astype(np.uint8)
    atlas = rng.randint(0, 256, 1500).astype(np.uint8)
    atlas[::7] = 255
    atlas[3::11] = 0
    return small, raw, filt, atlas


def random_marks(n, ph, pw, n_atlas, seed, per_frame=10):
    """Per frame up to per_frame marks of every kind, on every panel, in and across the panel's edges; maps cycle, one frame in five
    has no map (-1 or n_maps)."""
    rng = np.random.RandomState(seed)
    rows, first = [], [0]
    for f in range(n):
        for _ in range(rng.randint(0, per_frame + 1)):
            kind, panel = int(rng.randint(0, 4)), int(rng.randint(0, 5))
            x0, x1 = (int(v) for v in rng.randint(-6, pw + 6, 2))
            y0, y1 = (int(v) for v in rng.randint(-6, ph + 6, 2))
            rgb = tuple(int(v) for v in rng.randint(0, 256, 3))
            if kind == TEXT:
                sw, sh = int(rng.randint(1, 20)), int(rng.randint(1, 12))
                rows.append(mark(TEXT, panel, x0, y0, 0, 0, int(rng.randint(0, n_atlas - 100)), sw | sh << 16, rgb))
            elif kind == RECT:
                rows.append(mark(RECT, panel, min(x0, x1), min(y0, y1), max(x0, x1), max(y0, y1), 0, 0, rgb))
            else:
                rows.append(mark(kind, panel, x0, y0, x1, y1, int(rng.randint(0, 9)), 0, rgb))
        first.append(len(rows))
    return np.asarray(rows, np.int32).reshape(-1, WORDS), np.asarray(first, np.int32)


def edge_marks(kind, panel, ph, pw):
    """Marks of one kind on one panel: wholly inside, then across the left, right, top and bottom edge and every corner."""
    cx, cy = pw // 2, ph // 2
    spots = [(cx, cy), (0, cy), (pw - 1, cy), (cx, 0), (cx, ph - 1), (-1, -1), (pw, -1), (-1, ph), (pw, ph)]
    rows = []
    for i, (x, y) in enumerate(spots):
        rgb = (40 + 20 * i, 250 - 25 * i, 7 * i)
        if kind == DISC:
            rows.append(mark(DISC, panel, x, y, 0, 0, 3, 0, rgb))
        elif kind == LINE:
            rows.append(mark(LINE, panel, x - 4, y - 2, x + 4, y + 3, 3, 0, rgb))
        elif kind == RECT:
            rows.append(mark(RECT, panel, x - 3, y - 2, x + 3, y + 2, 0, 0, rgb))
        else:
            rows.append(mark(TEXT, panel, x - 4, y - 3, 0, 0, 13 * i, 9 | 6 << 16, rgb))
    return rows


def special_frames(ph, pw, n_atlas):
    """Named mark lists, one frame each (every list at most 64 marks unless it says otherwise)."""
    cx, cy = pw // 2, ph // 2
    red, green, blue, white = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    F = {}
    F['zero_length_line'] = [mark(LINE, 2, cx, cy, cx, cy, 5, 0, red), mark(LINE, 0, 1, 1, 1, 1, 1, 0, green), mark(LINE, 4, 2, 2, 2, 2, 0, 0, blue)]
    F['p_zero'] = [mark(DISC, 1, cx, cy, 0, 0, 0, 0, red), mark(LINE, 3, 0, 0, pw - 1, ph - 1, 0, 0, green), mark(LINE, 2, 1, cy, pw - 2, cy, 0, 0, blue)]
    F['p_255'] = [mark(DISC, 0, cx, cy, 0, 0, 255, 0, red), mark(LINE, 4, cx, cy, cx + 3, cy + 1, 255, 0, green),
                  mark(DISC, 2, -200, -150, 0, 0, 255, 0, blue)]
    F['long_line'] = [mark(LINE, 1, -90, -120, 90, 120, 3, 0, red), mark(LINE, 3, cx - 150, cy, cx + 150, cy, 2, 0, green),
                      mark(LINE, 2, 0, 0, 180, 240, 1, 0, blue), mark(LINE, 0, -32767, -32767, 32767, 32767, 4, 0, white)]
    F['sprite_partly_outside'] = [mark(TEXT, 0, pw - 4, 1, 0, 0, 0, 10 | 5 << 16, white), mark(TEXT, 4, -6, ph - 2, 0, 0, 50, 12 | 6 << 16, red),
                                  mark(TEXT, 2, -3, -2, 0, 0, 7, 8 | 8 << 16, green)]
    F['sprite_beyond_atlas'] = [mark(TEXT, 1, 0, 0, 0, 0, n_atlas - 20, 8 | 6 << 16, white), mark(TEXT, 3, 1, 1, 0, 0, -5, 4 | 4 << 16, red),
                                mark(TEXT, 2, 0, 0, 0, 0, n_atlas, 3 | 3 << 16, green), mark(TEXT, 0, 0, 0, 0, 0, 2 ** 31 - 1, 4096 | 4096 << 16, blue)]
    F['ignored'] = [mark(9, 0, cx, cy, 0, 0, 3, 0, red), mark(DISC, 5, cx, cy, 0, 0, 3, 0, red), mark(DISC, 1, 40000, cy, 0, 0, 3, 0, red),
                    mark(DISC, 1, cx, -40000, 0, 0, 3, 0, red), mark(RECT, 1, 0, 0, 40000, 3, 0, 0, red), mark(LINE, 2, 0, 0, 3, -32768, 1, 0, red),
                    mark(DISC, 2, cx, cy, 0, 0, 256, 0, red), mark(LINE, 2, 0, 0, 5, 5, 256, 0, red), mark(DISC, 3, cx, cy, 0, 0, -1, 0, red),
                    mark(TEXT, 3, 0, 0, 0, 0, 0, 4097 | 2 << 16, red), mark(TEXT, 3, 0, 0, 0, 0, 0, 2 | 4097 << 16, red),
                    mark(TEXT, 3, 0, 0, 0, 0, 0, -1, red), [-1, cx, cy, 0, 0, 3, 0, 255], [DISC | 1 << 30, cx, cy, 0, 0, 3, 0, 255],
                    mark(DISC, 4, 1, 1, 0, 0, 1, 0, green)]                       # (the last one applies)
    F['seventy'] = [mark(DISC, i % 5, (3 * i) % pw, (2 * i) % ph, 0, 0, 1, 0, (3 * i, 255 - 3 * i, 100)) for i in range(64)] + \
                   [mark(DISC, i % 5, cx, cy, 0, 0, 4, 0, white) for i in range(6)]      # 70: the last six must not show
    F['overlap'] = [mark(DISC, 2, cx, cy, 0, 0, 4, 0, red), mark(DISC, 2, cx + 1, cy, 0, 0, 3, 0, green), mark(TEXT, 2, cx - 4, cy - 2, 0, 0, 20, 9 | 5 << 16, blue),
                    mark(RECT, 2, cx - 2, cy - 2, cx + 2, cy + 2, 0, 0, white), mark(LINE, 2, 0, cy, pw, cy, 1, 0, (9, 8, 7))]
    return F


def frames_of(lists):
    rows, first = [], [0]
    for marks in lists:
        rows += marks
        first.append(len(rows))
    return np.asarray(rows, np.int64).astype(np.int32).reshape(-1, WORDS), np.asarray(first, np.int32)
