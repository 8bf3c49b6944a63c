"""Host restatement and fixtures shared by tests/test_flatten_cpu.py, tests/test_svg_cpu.py, tests/test_gpu_flatten.py and
tests/test_gpu_svg.py: the path-flattening rule of include/skf.h (Path flattening) in numpy.  The number of pieces of a cubic is
the smallest n in [1, 4096] with n^4 * c >= dd, c = (16 / 9) * tol^2, every float64 operation rounded on its own; a row is a copied
control point or six float64 lerps a coordinate in a fixed order, then one rounding to float32.  `bernstein` evaluates a cubic by
its polynomial in float64: the yardstick of the error bound, not part of the rule."""
import numpy as np

MAX_N = 4096                              # SKF_FLATTEN_MAX_N of include/skf.h
_N4 = np.arange(1, MAX_N + 1, dtype=np.float64) ** 2
_N4 = _N4 * _N4                           # (double)(n * n) * (double)(n * n), exact


def c_of(tol):
    """c = (16 / 9) * tol^2: the quotient, tol * tol, then their product, each rounded to float64"""
    tol = np.float64(tol)
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("tol must be finite and above 0")
    with np.errstate(over="ignore", under="ignore"):
        return (np.float64(16.0) / np.float64(9.0)) * (tol * tol)


def pieces(ctrl, kind, tol):
    """ctrl (G, 4, 2) float64, kind (G,) -> n (G,) int64"""
    p = np.asarray(ctrl, np.float64).reshape(-1, 4, 2)
    kind = np.asarray(kind).reshape(-1)
    c = c_of(tol)
    with np.errstate(all="ignore"):
        a = (p[:, 0] - 2.0 * p[:, 1]) + p[:, 2]
        b = (p[:, 1] - 2.0 * p[:, 2]) + p[:, 3]
        dd = np.maximum(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1], b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])      # a NaN stays a NaN
        # n^4 c is non-decreasing in n: the first entry >= dd is found by bisection; a NaN or an infinite dd sorts behind them all
        n = np.minimum(np.searchsorted(_N4 * c, dd, side="left") + 1, MAX_N).astype(np.int64)
    return np.where(kind == 1, n, 1)


def _lerp(a, b, t):
    return a + t * (b - a)


def segment_rows(p, n):
    """The n rows j = 1 .. n of one segment with the control points p (4, 2) -> float32 (n, 2)"""
    p = np.asarray(p, np.float64)
    out = np.empty((n, 2), np.float32)
    if n > 1:
        t = (np.arange(1, n, dtype=np.float64) / np.float64(n))[:, None]
        q0, q1, q2 = _lerp(p[0], p[1], t), _lerp(p[1], p[2], t), _lerp(p[2], p[3], t)
        r0, r1 = _lerp(q0, q1, t), _lerp(q1, q2, t)
        out[:n - 1] = _lerp(r0, r1, t).astype(np.float32)
    out[n - 1] = p[3].astype(np.float32)
    return out


def flatten_subpath(ctrl, kind, tol):
    """One subpath -> float32 (1 + sum n, 2); no segment gives no row"""
    p = np.asarray(ctrl, np.float64).reshape(-1, 4, 2)
    if len(p) == 0:
        return np.zeros((0, 2), np.float32)
    n = pieces(p, kind, tol)
    return np.concatenate([p[0, :1].astype(np.float32)] + [segment_rows(p[k], int(n[k])) for k in range(len(p))], axis=0)


def flatten(ctrl, kind, path_offsets, tol):
    """The batch, subpath by subpath, the ranges clamped to [0, G] as skf_ragged_range clamps them -> list of float32 (rows, 2)"""
    p = np.asarray(ctrl, np.float64).reshape(-1, 4, 2)
    kind = np.asarray(kind).reshape(-1)
    G, out = len(p), []
    for s in range(len(path_offsets) - 1):
        beg = min(max(int(path_offsets[s]), 0), G)
        end = min(max(int(path_offsets[s + 1]), beg), G)
        out.append(flatten_subpath(p[beg:end], kind[beg:end], tol))
    return out


def pack(parts):
    """list of (n, 2) float32 -> (xy (P', 2), offsets int64)"""
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    xy = np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(xy, dtype=np.float32), offsets


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def bernstein(p, t):
    """The cubic with the control points p (4, 2) at the parameters t -> float64 (len(t), 2)"""
    p = np.asarray(p, np.float64)
    t = np.asarray(t, np.float64)[:, None]
    u = 1.0 - t
    return u * u * u * p[0] + 3.0 * u * u * t * p[1] + 3.0 * u * t * t * p[2] + t * t * t * p[3]


def deviation(p, n):
    """The largest distance from the dense float64 curve (20 n + 1 samples) to the float32 polyline of the segment's n pieces"""
    p = np.asarray(p, np.float64)
    poly = np.concatenate([p[:1].astype(np.float32), segment_rows(p, n)]).astype(np.float64)
    dense = bernstein(p, np.arange(20 * n + 1, dtype=np.float64) / (20 * n))
    piece = np.minimum(np.arange(20 * n + 1) // 20, n - 1)                      # sample i lies on piece i // 20
    a, b = poly[piece], poly[piece + 1]
    e = b - a
    len2 = (e * e).sum(axis=1)
    w = dense - a
    u = np.clip((w * e).sum(axis=1) / np.where(len2 > 0, len2, 1.0), 0.0, 1.0)
    r = w - u[:, None] * e
    return float(np.sqrt((r * r).sum(axis=1)).max())


# ---------------------------------------------------------------- fixtures
def line_segment(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.stack([a, a, b, b])


def bump(n, tol):
    """A cubic whose piece count at `tol` is exactly n >= 2: both second differences are (0, h), with h^2 halfway between
    (n - 1)^4 c and n^4 c"""
    c = float(c_of(tol))
    h = np.sqrt(0.5 * (float(n - 1) ** 4 + float(n) ** 4) * c)
    return np.array([(0.0, 0.0), (1.0, -h), (2.0, -h), (3.0, 0.0)], np.float64)


def random_cubics(count, seed=51, size=800.0):
    rng = np.random.RandomState(seed)
    return rng.uniform(0, size, size=(count, 4, 2))


def random_subpaths(lengths, seed=52, size=800.0, line_every=0):
    """Connected subpaths of the given numbers of segments -> (ctrl, kind, path_offsets); every line_every-th segment is a line"""
    rng = np.random.RandomState(seed)
    ctrl, kind = [], []
    for g in lengths:
        at = rng.uniform(0, size, size=2)
        for k in range(g):
            step = rng.uniform(-60, 60, size=(3, 2))
            p = np.stack([at, at + step[0], at + step[0] + step[1], np.clip(at + step[0] + step[1] + step[2], 0, size)])
            is_line = bool(line_every) and (len(kind) % line_every == 0)
            ctrl.append(p)
            kind.append(0 if is_line else 1)
            at = p[3]
    offsets = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    ctrl = np.array(ctrl, np.float64).reshape(-1, 4, 2)
    return ctrl, np.array(kind, np.int32), offsets
