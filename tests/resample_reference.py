"""Host restatement and fixtures shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py: the arc-length resampling
rule of include/skf.h (Arc-length resampling of polylines) in numpy.  Segment lengths are fp32, one rounding per operation, and
are fixed to int64 in units of 2^-16; the table, the targets and the choice of a segment are integer work; a sample is three
float64 operations, then one rounding to float32.  `count_targets_exact` restates the count-mode targets with Python integers."""
import numpy as np

UNIT = 65536                              # arc lengths are integers in units of 2^-16
MAX_COORD = 16384                         # SKF_RESAMPLE_MAX_COORD of include/skf.h
MAX_N = 65536                             # SKF_RESAMPLE_MAX_N


def step_of(spacing):
    """s = rint(spacing * 2^16) as a Python integer; ValueError below 1"""
    s = np.float64(spacing) * np.float64(UNIT)
    if not np.isfinite(s) or np.rint(s) < 1:
        raise ValueError("spacing must be finite with rint(spacing * 2^16) >= 1")
    return int(np.rint(s))


def arc_table(xy):
    """(n, 2) points -> (q int64 (n - 1,), C int64 (n,)): the fixed segment lengths and their running sum from 0"""
    p = np.asarray(xy, np.float32).reshape(-1, 2)
    d = p[1:] - p[:-1]
    assert d.dtype == np.float32
    c = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    assert c.dtype == np.float32
    q = np.rint(c.astype(np.float64) * np.float64(UNIT)).astype(np.int64)
    return q, np.concatenate([np.zeros(1, np.int64), np.cumsum(q, dtype=np.int64)])


def n_rows(total, step):
    """ceil(total / step) + 1"""
    return -(-int(total) // int(step)) + 1


def sample(xy, q, C, T):
    """The samples at the int64 targets T (all below C[-1]) -> float32 (len(T), 2)"""
    p = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    T = np.asarray(T, np.int64)
    i = np.searchsorted(C, T, side="right") - 1                                # C_i <= T < C_{i+1}
    u = (T - C[i]).astype(np.float64) / q[i].astype(np.float64)
    prod = u[:, None] * (p[i + 1] - p[i])
    return (p[i] + prod).astype(np.float32)


def spacing_targets(total, step):
    return np.arange(n_rows(total, step) - 1, dtype=np.int64) * np.int64(step)


def count_targets(total, n_out):
    """T_m = m * a + (m * r) // (n_out - 1), m = 0 .. n_out - 2, in int64"""
    last = n_out - 1
    a, r = int(total) // last, int(total) % last
    m = np.arange(last, dtype=np.int64)
    return m * np.int64(a) + (m * np.int64(r)) // np.int64(last)


def count_targets_exact(total, n_out):
    return [m * int(total) // (n_out - 1) for m in range(n_out - 1)]


def resample(xy, spacing):
    """Spacing mode: (n, 2) -> float32 (ceil(total / s) + 1, 2); no point gives no row"""
    p = np.asarray(xy, np.float32).reshape(-1, 2)
    step = step_of(spacing)
    if len(p) == 0:
        return np.zeros((0, 2), np.float32)
    q, C = arc_table(p)
    return np.concatenate([sample(p, q, C, spacing_targets(C[-1], step)), p[-1:]], axis=0)


def resample_n(xy, n_out):
    """Count mode: (n, 2) -> float32 (n_out, 2); no point gives n_out rows (0, 0), total == 0 gives n_out copies of the first"""
    p = np.asarray(xy, np.float32).reshape(-1, 2)
    if not 2 <= n_out <= MAX_N:
        raise ValueError("n_out must be in [2, %d]" % MAX_N)
    if len(p) == 0:
        return np.zeros((n_out, 2), np.float32)
    q, C = arc_table(p)
    if C[-1] == 0:
        return np.repeat(p[:1], n_out, axis=0)
    return np.concatenate([sample(p, q, C, count_targets(C[-1], n_out)), p[-1:]], axis=0)


def resample_all(lines, spacing):
    return [resample(l, spacing) for l in lines]


def pack(parts):
    """list of (n, 2) float32 -> (xy (P', 2), offsets int64)"""
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    xy = np.concatenate(parts, axis=0) if parts else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(xy, dtype=np.float32), offsets


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- fixtures
LINE_0_10 = np.array([(0, 0), (10, 0)], np.float32)
PYTHAGORAS = np.array([(0, 0), (3, 4), (6, 0), (6, 5), (9, 9)], np.float32)      # every segment has length 5


def split_at_midpoints(xy):
    """every segment split at its midpoint (exactly representable for the fixtures that use it)"""
    p = np.asarray(xy, np.float32)
    mid = (p[:-1] + p[1:]) * np.float32(0.5)
    out = np.empty((2 * len(p) - 1, 2), np.float32)
    out[0::2], out[1::2] = p, mid
    return out


def random_int_strokes(count, seed=41):
    """count strokes of 2 .. 60 integer points in 0 .. 255"""
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(int(rng.randint(2, 61)), 2)).astype(np.float32) for _ in range(count)]
