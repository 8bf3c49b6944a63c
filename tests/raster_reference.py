"""float64 numpy restatements of the three definitions of include/skf.h's "Sketches as images" block: the point decoders
(written from the definitions, one position at a time), the rasterizer and the overlap sums.  `rasterize` takes the dtype of its
arithmetic as an argument: float64 is the reference, float32 the same formula in the precision of the kernel."""
import numpy as np


# ---------------------------------------------------------------- points
def _finish(offsets, pens, absolute=False):
    if not offsets:
        return np.zeros((0, 2)), np.zeros(0, np.uint8)
    xy = np.array(offsets, dtype=np.float64)
    if not absolute:
        xy = np.cumsum(xy, axis=0)
    return xy, np.array(pens, dtype=np.uint8)


def points_stroke3(rows, length):
    rows = np.asarray(rows)
    n = min(max(int(length), 0), len(rows))
    return _finish([[float(r[0]), float(r[1])] for r in rows[:n]], [int(r[2] == 1) for r in rows[:n]])


def points_stroke5(rows):
    offs, pens = [], []
    for r in np.asarray(rows):
        a = 0
        for k in (1, 2):                                 # ties go to the first index
            if r[2 + k] > r[2 + a]:
                a = k
        if a == 2:
            break
        offs.append([float(r[0]), float(r[1])])
        pens.append(int(a == 1))
    return _finish(offs, pens)


def points_dict(tokens, centers):
    K = len(centers)
    SEP, EOS = K + 1, K + 3
    offs, pens = [], []
    for t in np.asarray(tokens).reshape(-1):
        t = int(t)
        if 1 <= t <= K:
            offs.append([float(centers[t - 1][0]), float(centers[t - 1][1])])
            pens.append(0)
        elif t == SEP and pens:
            pens[-1] = 1
        elif t == EOS:
            break                                        # PAD, SOS and ids outside the vocabulary: skipped
    return _finish(offs, pens)


def points_grid(tokens, resolution):
    R = int(resolution)
    r = R // 2
    n = R * R
    SEP, EOS = n + 1, n + 3
    pts, pens = [], []
    for t in np.asarray(tokens).reshape(-1):
        t = int(t)
        if 1 <= t <= n:
            pts.append([((t - 1) % R) / r - 1 + 1 / R, ((t - 1) // R) / r - 1 + 1 / R])
            pens.append(0)
        elif t == SEP and pens:
            pens[-1] = 1
        elif t == EOS:
            break
    if pens:
        pens[-1] = 1                                     # the host decoder closes its last line
    return _finish(pts, pens, absolute=True)


def bounds(xy):
    if len(xy) == 0:
        return np.zeros(4)
    return np.r_[xy.min(0), xy.max(0)]


# ---------------------------------------------------------------- raster
def frame_scale(frame, H, W, margin, dt=np.float64):
    """-> (s, box centre x, box centre y) of the frame rule, every operation in dt"""
    x0, y0, x1, y1 = (dt(v) for v in frame)
    w, h = dt(x1 - x0), dt(y1 - y0)
    m2 = dt(dt(2) * dt(margin))
    cand = []
    if w >= dt(1e-6):
        cand.append(dt(dt(dt(W) - m2) / w))
    if h >= dt(1e-6):
        cand.append(dt(dt(dt(H) - m2) / h))
    s = min(cand) if cand else dt(0)
    return s, dt(dt(0.5) * dt(x0 + x1)), dt(dt(0.5) * dt(y0 + y1))


def to_pixels(xy, frame, H, W, margin, dt=np.float64):
    s, cx, cy = frame_scale(frame, H, W, margin, dt)
    p = np.asarray(xy).astype(dt).reshape(-1, 2)
    q = np.empty_like(p)
    q[:, 0] = dt(0.5) * dt(W) + s * (p[:, 0] - cx)
    q[:, 1] = dt(0.5) * dt(H) + s * (p[:, 1] - cy)
    return q


def rasterize(xy, pen, frame, H, W, line_width=1.5, margin=2.0, dt=np.float64, chunk=32, centred=False):
    """One sketch (absolute points xy (n, 2), pen (n,)) -> its (H, W) coverage image.  centred: the same formula with points and
    pixel centres both taken relative to the canvas centre (W / 2, H / 2) - the arrangement of the kernel: the distances are the
    same, the coordinates half as large and one addition shorter."""
    n = len(xy)
    if n == 0:
        return np.zeros((H, W), dtype=dt)
    q = to_pixels(xy, frame, H, W, margin, dt)
    ox, oy = dt(0), dt(0)
    if centred:
        s, bx, by = frame_scale(frame, H, W, margin, dt)
        p = np.asarray(xy).astype(dt).reshape(-1, 2)
        q = np.stack([s * (p[:, 0] - bx), s * (p[:, 1] - by)], axis=1)
        ox, oy = dt(0.5) * dt(W), dt(0.5) * dt(H)
    pen = np.asarray(pen)
    a = q.copy()
    if n > 1:
        a[1:] = np.where((pen[:-1] == 0)[:, None], q[:-1], q[1:])
    d = q - a
    l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    inv = np.where(l2 > 0, dt(1) / np.where(l2 > 0, l2, dt(1)), dt(0)).astype(dt)
    cx = ((np.arange(W).astype(dt) + dt(0.5)) - ox)[None, :, None]
    cy = ((np.arange(H).astype(dt) + dt(0.5)) - oy)[:, None, None]
    best = np.full((H, W), np.inf, dtype=dt)
    for i in range(0, n, chunk):
        ax, ay, dx, dy, iv = (v[None, None, i:i + chunk] for v in (a[:, 0], a[:, 1], d[:, 0], d[:, 1], inv))
        rx, ry = cx - ax, cy - ay
        t = np.clip((rx * dx + ry * dy) * iv, dt(0), dt(1))
        # e = r - t d is ONE fused multiply-add in the kernel (t d is as long as the segment, e as short as the distance: rounding
        # the product would cost an error of the segment's magnitude); a float32 product is exact in float64, so this is fmaf
        ex = (rx.astype(np.float64) - t.astype(np.float64) * dx).astype(dt)
        ey = (ry.astype(np.float64) - t.astype(np.float64) * dy).astype(dt)
        best = np.minimum(best, (ex * ex + ey * ey).min(-1))
    assert best.dtype == dt
    return np.clip(dt(0.5) + dt(0.5) * dt(line_width) - np.sqrt(best), dt(0), dt(1))


def raster_bound(H, W):
    """per pixel: coverage is 1-Lipschitz in the pixel-space coordinates; 32 roundings at the magnitude of the largest one"""
    return 32.0 * 2.0 ** -24 * max(H, W)


# ---------------------------------------------------------------- overlap
def overlap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array([np.minimum(a, b).sum(), np.maximum(a, b).sum()])


def soft_iou(a, b):
    lo, hi = overlap(a, b)
    return lo / hi if hi > 0 else 1.0


# ---------------------------------------------------------------- shared inputs
def dyadic_walk(n, seed, step=64):
    """(n, 2) offsets, multiples of 2^-10 of at most step * 2^-10 a side: every partial sum is a multiple of 2^-10 below 4 and so
    exact in float32"""
    rng = np.random.RandomState(seed)
    off = rng.randint(-step, step + 1, size=(n, 2)).astype(np.float64) / 1024.0
    assert np.abs(np.cumsum(off, axis=0)).max() <= 4.0
    return off


def dyadic_sketches(lengths, seed, pen_rate=0.15):
    """[(xy (n, 2) float64 exact in float32, pen (n,) uint8)] of random walks"""
    rng = np.random.RandomState(seed + 1000)
    out = []
    for k, n in enumerate(lengths):
        xy = np.cumsum(dyadic_walk(n, seed + k), axis=0)
        out.append((xy, (rng.rand(n) < pen_rate).astype(np.uint8)))
    return out


def pack_points(sketches):
    """[(xy, pen)] -> xy (B, T, 2) float32, pen (B, T) uint8, n (B,) int32, bounds (B, 4) float32"""
    B, T = len(sketches), max(1, max(len(s[0]) for s in sketches))
    xy, pen = np.zeros((B, T, 2), np.float32), np.zeros((B, T), np.uint8)
    n, bnd = np.zeros(B, np.int32), np.zeros((B, 4), np.float32)
    for i, (p, q) in enumerate(sketches):
        xy[i, :len(p)], pen[i, :len(p)], n[i], bnd[i] = p, q, len(p), bounds(p)
        assert np.array_equal(xy[i, :len(p)].astype(np.float64), p)
    return xy, pen, n, bnd


# the raster cases both the CPU check of the float32 restatement and the GPU test walk: (H, W), sketch lengths
RASTER_SHAPES = (((24, 40), (1, 7, 65)), ((64, 64), (2, 64, 300)), ((256, 256), (65, 130)))
LINE_WIDTHS = (1.0, 1.5, 9.0)
FIXED_FRAME = (-0.25, -0.125, 0.5, 0.375)       # cuts through the walks: part of every longer sketch lies outside the canvas


# ---------------------------------------------------------------- token / stroke rows for the point decoders
POINT_LENGTHS = (1, 2, 63, 64, 65, 300)          # the wave edges and one carry across chunks


def token_cases(T, nid, seed):
    """{name: (T,) int64 row} over a vocabulary of ids 1 .. nid, SEP = nid + 1, SOS = nid + 2, EOS = nid + 3"""
    rng = np.random.RandomState(seed)
    SEP, SOS, EOS = nid + 1, nid + 2, nid + 3
    ids = lambda: rng.randint(1, nid + 1, size=T).astype(np.int64)           # noqa: E731
    out = {}
    row = ids()
    row[rng.rand(T) < 0.15] = SEP
    row[0] = SOS
    if T >= 3:
        row[-1] = EOS
    out["plain"] = row
    row = ids()
    row[rng.rand(T) < 0.1] = SEP
    row[T // 2] = EOS                                                         # what follows must not be read as points
    out["eos_middle"] = row
    out["no_sep"] = ids()
    row = ids()
    row[:min(2, T)] = SEP                                                     # separators before any point lift nothing
    for at in (5, 6, 20, 21, 22, 63, 64, 130, 191, 192, 193, T - 1):          # pairs, a triple, one pair across the chunk edge
        if 0 <= at < T:
            row[at] = SEP
    out["consecutive_seps"] = row
    out["all_pad"] = np.zeros(T, dtype=np.int64)
    row = ids()
    for at, bad in ((0, nid + 4), (1, -1), (7, nid + 100), (63, -5), (64, 1 << 40), (200, nid + 4)):
        if at < T:
            row[at] = bad
    row[rng.rand(T) < 0.1] = SEP
    out["out_of_vocab"] = row
    return out


def stroke5_cases(T, seed):
    """{name: (T, 5) float32}: dyadic offsets, pen logits with ties"""
    rng = np.random.RandomState(seed)

    def rows():
        r = np.zeros((T, 5), dtype=np.float32)
        r[:, :2] = dyadic_walk(T, seed + 7)
        state = rng.choice(2, size=T, p=[0.85, 0.15])
        r[np.arange(T), 2 + state] = 1.0
        r[:, 2:] += rng.choice([0.0, 0.25], size=(T, 3)).astype(np.float32) * (1 - np.eye(3, dtype=np.float32)[state]) * 0.5
        tie = rng.rand(T) < 0.1
        r[tie, 2:] = 0.5                                                       # a three-way tie: index 0, pen down
        return r
    out = {"no_end": rows()}
    r = rows()
    r[T // 2, 2:] = (0.0, 0.0, 1.0)
    out["end_middle"] = r
    r = rows()
    r[0, 2:] = (0.25, 0.25, 1.0)
    out["end_first"] = r
    r = rows()
    r[T - 1, 2:] = (0.0, 1.0, 1.0)                                             # tie between lift and end: lift wins
    out["tie_lift_end"] = r
    return out


def dyadic_centers(K, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(-48, 49, size=(K, 2)).astype(np.float64) / 1024.0).astype(np.float32)
