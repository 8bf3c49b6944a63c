"""Host references and fixtures shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py.  The host side is the project's
own DistributedStroke3DataLoader._augment_sketch, fed with chosen draws through a stand-in for np.random.random; `restate` is the
rule of include/skf.h as a plain loop, with three switches that make it wrong on purpose - they give the GPU tests their teeth:
  (a) sum_first:    a run of dropped points is summed first and the sum added to the kept row (one rounding less per point);
  (b) fp32_draws:   the draw is rounded to fp32 before it is compared with prob;
  (c) fp32_factors: the scale factors are evaluated in fp32 instead of float64."""
import numpy as np

from preprocess_reference import host_loader
from simplify_reference import OFFSETS_SCAN_BLOCK       # noqa: F401  (the block width of the offsets scan both pipelines share)
from sketchformer_amd import preprocess


class _Replay:
    """np.random.random, replaying an array: () -> the next draw as a Python float, (size=n) -> the next n draws."""

    def __init__(self, rnd):
        self.rnd, self.pos = np.asarray(rnd, np.float64), 0

    def __call__(self, size=None):
        n = 1 if size is None else int(size)
        got = self.rnd[self.pos:self.pos + n].copy()
        assert len(got) == n, "the host asked for more draws than the stream holds"
        self.pos += n
        return float(got[0]) if size is None else got


def n_draws(sketches):
    return 2 * len(sketches) + int(sum(len(s) for s in sketches))


def host_augment(sketches, rnd, scale_factor, prob, clamp=True):
    """_augment_sketch of every sketch, in order, under the draws `rnd` (2 N + P of them, all consumed) -> list of float32 (n', 3)."""
    loader = host_loader(use_continuous_data=True, augment_stroke_prob=prob, random_scale_factor=scale_factor)
    replay, saved = _Replay(rnd), np.random.random
    np.random.random = replay
    try:
        out = []
        for s in sketches:
            s32 = np.array(np.clip(s, -1000, 1000) if clamp else s, dtype=np.float32).reshape(-1, 3)
            out.append(np.asarray(loader._augment_sketch(s32), np.float32).reshape(-1, 3))
    finally:
        np.random.random = saved
    assert replay.pos == len(replay.rnd) == n_draws(sketches)
    return out


def packed(sketches):
    """list of (n, 3) arrays -> (flat float32 (P, 3), offsets int64 (N + 1)), read-only."""
    flat, offsets = preprocess.pack_ragged(sketches)
    flat.setflags(write=False)
    offsets.setflags(write=False)
    return flat, offsets


def restate(sketch, draws, scale_factor, prob, clamp=True, sum_first=False, fp32_draws=False, fp32_factors=False):
    """One sketch by the rule of include/skf.h as a plain loop; draws = (ux, uy, one per point).  With every switch off this is
    the host's result (tests/test_augment_cpu.py asserts that)."""
    f32 = np.float32
    s = np.array(np.clip(sketch, -1000, 1000) if clamp else sketch, dtype=np.float32).reshape(-1, 3)
    ux, uy, u = float(draws[0]), float(draws[1]), np.asarray(draws[2:], np.float64)
    assert len(u) == len(s)
    if fp32_factors:
        fx = (f32(ux) - f32(0.5)) * f32(2) * f32(scale_factor) + f32(1)
        fy = (f32(uy) - f32(0.5)) * f32(2) * f32(scale_factor) + f32(1)
        assert fx.dtype == np.float32
    else:
        fx, fy = f32((ux - 0.5) * 2.0 * scale_factor + 1.0), f32((uy - 0.5) * 2.0 * scale_factor + 1.0)
    x, y = s[:, 0] * fx, s[:, 1] * fy
    rows, prev, count, run = [], 1.0, 0, None
    for t in range(len(s)):
        pen = float(s[t, 2])
        count = 0 if (pen == 1 or prev == 1) else count + 1
        ut = float(f32(u[t])) if fp32_draws else float(u[t])
        if pen == 0 and prev == 0 and count > 2 and ut < prob:
            if sum_first:
                run = [x[t], y[t]] if run is None else [run[0] + x[t], run[1] + y[t]]
            else:
                rows[-1][0], rows[-1][1] = rows[-1][0] + x[t], rows[-1][1] + y[t]
            continue
        if run is not None:
            rows[-1][0], rows[-1][1], run = rows[-1][0] + run[0], rows[-1][1] + run[1], None
        rows.append([x[t], y[t], s[t, 2]])
        prev = pen
    if run is not None:
        rows[-1][0], rows[-1][1] = rows[-1][0] + run[0], rows[-1][1] + run[1]
    return np.array(rows, dtype=np.float32).reshape(-1, 3)


def restate_all(sketches, rnd, scale_factor, prob, **kw):
    out, pos = [], 0
    for s in sketches:
        out.append(restate(s, rnd[pos:pos + 2 + len(s)], scale_factor, prob, **kw))
        pos += 2 + len(s)
    assert pos == len(rnd)
    return out


def n_differing(a, b):
    return sum(1 for p, q in zip(a, b) if p.shape != q.shape or not np.array_equal(p, q))


# ---------------------------------------------------------------- fixtures: (sketches, rnd, scale_factor, prob)
def order_fixture(n=200):
    """(a) Integer sketches of 8 - 60 points, offsets within +-40, one lift at the end, scaled by an fp32 factor, prob = 0.9: long
    runs of dropped points whose fp32 sum depends on whether the run is added point by point or as one sum."""
    rng = np.random.RandomState(20250101)
    sketches = []
    for _ in range(n):
        m = int(rng.randint(8, 61))
        s = np.zeros((m, 3), np.int16)
        s[:, :2] = rng.randint(-40, 41, size=(m, 2))
        s[-1, 2] = 1
        sketches.append(s)
    return sketches, rng.random_sample(n_draws(sketches)), 0.1, 0.9


def threshold_fixture():
    """(b) One draw just below prob = 0.1 on a droppable point: below in float64, not below once rounded to fp32."""
    u = np.nextafter(0.1, 0)
    assert u < 0.1 and not float(np.float32(u)) < 0.1
    s = np.array([[3, 1, 0], [-2, 5, 0], [7, -4, 0], [1, 1, 0], [2, 2, 0], [-6, 3, 1]], np.int16)
    rnd = np.array([0.5, 0.5, 0.9, 0.9, 0.9, u, 0.9, 0.9])
    return [s, s.copy()], np.concatenate([rnd, rnd]), 0.0, 0.1


def factor_fixture():
    """(c) 32 sketches whose 64 scale draws come from RandomState(5); nothing is dropped (every point draw is 0.99, prob 0.1)."""
    draws = np.random.RandomState(5).random_sample(64)
    rng = np.random.RandomState(6)
    sketches, rnd = [], []
    for i in range(32):
        s = np.zeros((7, 3), np.int16)
        s[:, :2] = rng.randint(-40, 41, size=(7, 2))
        s[-1, 2] = 1
        sketches.append(s)
        rnd += [draws[2 * i], draws[2 * i + 1]] + [0.99] * 7
    return sketches, np.array(rnd), 0.1, 0.1


# ---------------------------------------------------------------- the sweep
LENGTHS = (1, 2, 3, 4, 5, 6, 64, 65, 230)


def sketch(rng, n, pen="random", lo=-40, hi=40, dtype=np.int16):
    s = np.zeros((n, 3), dtype=dtype)
    s[:, :2] = rng.randint(lo, hi + 1, size=(n, 2))
    if pen == "random":
        s[:, 2] = rng.rand(n) < 0.08
    if pen in ("random", "last"):
        s[-1, 2] = 1
    return s


def sweep_pool():
    """2 * OFFSETS_SCAN_BLOCK + 5 sketches: the named cases first (the first 130 hold all of them), short random ones behind them.
    Every count of the sweep takes a prefix."""
    rng = np.random.RandomState(17)
    pool = [sketch(rng, 65)]                                                   # N = 1: lifts in the middle, across a wave's width
    for n in LENGTHS:
        for pen in ("last", "random", "none"):                                 # none: a sketch with no lift at all
            pool.append(sketch(rng, n, pen=pen))
    s = sketch(rng, 40, pen="last")
    s[[9, 10, 25], 2] = 1                                                      # two lifts in a row, and one more
    pool.append(s)
    s = sketch(rng, 30, pen="last")
    s[12, 2] = 2                                                               # a pen value that is neither 0 nor 1
    pool.append(s)
    pool.append(np.array([[1500, -3000, 0], [-1200, 20, 0], [999, 1001, 0], [-1000, 5000, 0], [2000, -2000, 0], [1, 2, 0],
                          [3000, 1, 1500], [5, 5, 0], [7, 7, 1]], np.int32))          # beyond the clamp, the pen column included
    pool.append(np.array([[1500.5, -3000.25, 0], [3.5, 2000.0, 0], [0.5, 0.25, 0], [1e-3, -1e-3, 0], [-1000.5, 0.5, 0],
                          [0.125, 7.75, 1]], np.float64))
    pool.append(np.zeros((9, 3), np.int16))                                    # zero offsets
    while len(pool) < 130:
        pool.append(sketch(rng, int(rng.randint(1, 120))))
    while len(pool) < 2 * OFFSETS_SCAN_BLOCK + 5:
        pool.append(sketch(rng, int(rng.randint(1, 12))))
    return pool
