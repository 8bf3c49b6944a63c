"""Host restatement and fixtures shared by tests/test_simplify_cpu.py and tests/test_gpu_simplify.py.  `rdp_mask` is the rule of
include/skf.h (Stroke simplification) as an explicit-stack recursion in numpy float64; `simplify_stroke3` wraps it for stroke-3
sketches with sequential fp32 position sums; `rdp_mask_exact` evaluates the same rule in Python integers / fractions for
integer-valued points, with no rounding anywhere.  `last_max_wins` makes the restatement wrong on purpose: it gives the tie
fixture its teeth."""
import os
import runpy
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prepare_quickdraw")       # tools/record_prepare_quickdraw_golden.py wrote it
LDS_POINTS = 512                          # SKF_RDP_LDS_POINTS of include/skf.h: longer polylines run from the workspace
OFFSETS_SCAN_BLOCK = 1024                 # OFFS_THREADS of skf_ragged.hip: the counts go through the scan in tiles of this many


# ---------------------------------------------------------------- the rule
def rdp_mask(xy, epsilon, last_max_wins=False, return_depth=False):
    """(n, 2) points -> uint8 (n,) keep mask.  The points are taken as fp32 and widened to float64; every numpy operation below is
    rounded on its own.  With return_depth also the deepest call of the recursion, the root counted as 1 and the calls on segments
    without an interior included: the number of levels a level-synchronous evaluation runs, the last of which keeps nothing."""
    p = np.asarray(xy, np.float32).reshape(-1, 2).astype(np.float64)
    n = len(p)
    keep = np.zeros(n, np.uint8)
    if n:
        keep[0] = keep[n - 1] = 1
    eps2 = np.float64(epsilon) * np.float64(epsilon)
    depth = 1 if n >= 2 else 0
    stack = [(0, n - 1, 1)]
    while stack:
        a, b, level = stack.pop()
        depth = max(depth, level) if b > a else depth
        if b - a < 2:
            continue
        ex, ey = p[b, 0] - p[a, 0], p[b, 1] - p[a, 1]
        px, py = p[a + 1:b, 0] - p[a, 0], p[a + 1:b, 1] - p[a, 1]
        if ex == 0 and ey == 0:
            m, L2 = px * px + py * py, np.float64(1)
        else:
            c = ex * py - ey * px
            m, L2 = c * c, ex * ex + ey * ey
        k = (b - 1 - int(np.argmax(m[::-1]))) if last_max_wins else (a + 1 + int(np.argmax(m)))
        with np.errstate(over="ignore"):
            if m[k - a - 1] > eps2 * L2:
                keep[k] = 1
                stack += [(a, k, level + 1), (k, b, level + 1)]
    return (keep, depth) if return_depth else keep


def rdp_mask_exact(points, epsilon):
    """The same rule in Python integers: points must hold integers, epsilon anything a Fraction takes exactly."""
    pts = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()]
    assert np.array_equal(np.asarray(pts).reshape(-1, 2), np.asarray(points).reshape(-1, 2))
    n, eps2 = len(pts), Fraction(epsilon) * Fraction(epsilon)
    keep = [0] * n
    if n:
        keep[0] = keep[n - 1] = 1
    stack = [(0, n - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        (xa, ya), (xb, yb) = pts[a], pts[b]
        ex, ey = xb - xa, yb - ya
        if ex == 0 and ey == 0:
            m, L2 = [(x - xa) ** 2 + (y - ya) ** 2 for x, y in pts[a + 1:b]], 1
        else:
            m, L2 = [(ex * (y - ya) - ey * (x - xa)) ** 2 for x, y in pts[a + 1:b]], ex * ex + ey * ey
        best = max(m)
        k = a + 1 + m.index(best)
        if best > eps2 * L2:
            keep[k] = 1
            stack += [(a, k), (k, b)]
    return np.array(keep, np.uint8)


def absolute_f32(sketch):
    """The positions of a stroke-3 sketch: the sequential fp32 running sum of dx and of dy, one add per point, from (0, 0)."""
    s = np.asarray(sketch)[:, :2].astype(np.float32)
    out = np.empty_like(s)
    ax, ay = np.float32(0), np.float32(0)
    for j in range(len(s)):
        ax, ay = ax + s[j, 0], ay + s[j, 1]
        out[j, 0], out[j, 1] = ax, ay
    assert out.dtype == np.float32
    return out


def stroke_ranges(pen):
    """[(first, last + 1)] of the strokes: runs of rows that end at a row with pen == 1, or at the last row."""
    ends = [j + 1 for j in range(len(pen)) if pen[j] == 1]
    if len(pen) and (not ends or ends[-1] != len(pen)):
        ends.append(len(pen))
    return list(zip([0] + ends[:-1], ends))


def simplify_stroke3(sketch, epsilon, **kw):
    """One stroke-3 sketch by the rule of skf_stroke3_simplify -> float32 (n', 3)."""
    s = np.asarray(sketch)[:, :3].astype(np.float32).reshape(-1, 3)
    pos = absolute_f32(s)
    keep = np.zeros(len(s), bool)
    for lo, hi in stroke_ranges(s[:, 2]):
        keep[lo:hi] = rdp_mask(pos[lo:hi], epsilon, **kw) != 0
    out = np.zeros((int(keep.sum()), 3), np.float32)
    prev = np.zeros(2, np.float32)
    for r, j in enumerate(np.flatnonzero(keep)):
        out[r, :2] = pos[j] - prev
        out[r, 2] = s[j, 2]
        prev = pos[j]
    return out


def simplify_all(sketches, epsilon):
    return [simplify_stroke3(s, epsilon) for s in sketches]


def pack_lines(lines):
    """list of (n, 2) polylines -> (xy float32 (P, 2), offsets int64 (S + 1)), read-only."""
    lens = np.array([len(l) for l in lines], np.int64)
    offsets = np.zeros(len(lines) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    parts = [np.asarray(l, np.float32).reshape(-1, 2) for l in lines if len(l)]
    xy = np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0, 2), np.float32)
    xy.setflags(write=False)
    offsets.setflags(write=False)
    return xy, offsets


def masks(lines, epsilon):
    """The restatement's masks of the polylines, back to back."""
    parts = [rdp_mask(l, epsilon) for l in lines]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


# ---------------------------------------------------------------- named fixtures: (points, epsilon, mask)
TENT = (np.array([(0, 0), (2, 5), (4, 1), (6, 5), (8, 0)], np.float32), 4.5, [1, 1, 0, 0, 1])          # m ties at 1 and 3
SQUARE = (np.array([(10, 10), (20, 10), (20, 20), (10, 20), (10, 10)], np.float32), 2.0, [1, 1, 1, 1, 1])   # a closed segment
COLLINEAR = (np.array([(0, 0), (1, 1), (2, 2), (3, 3)], np.float32), 0.0, [1, 0, 0, 1])               # 0 > 0 is false
ZIGZAG_LENGTHS = (65, 130, 257)


def zigzag(n):
    """x = 2 i, y = (i odd) * (3 + n - i): the amplitude shrinks along the line, every level of the recursion peels one point."""
    i = np.arange(n)
    return np.stack([2 * i, (i % 2) * (3 + n - i)], axis=1).astype(np.float32)


# ---------------------------------------------------------------- the pools
STROKE_LENGTHS = (0, 1, 2, 3, 4, 63, 64, 65, 130, LDS_POINTS - 1, LDS_POINTS, LDS_POINTS + 1, LDS_POINTS + 5)


def smooth_int_stroke(rng, n):
    """A pen that turns slowly and moves 2 - 5 units a point, rounded to the integer grid: what RDP is there to thin out."""
    if n == 0:
        return np.zeros((0, 2), np.float32)
    heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.25, size=n))
    step = rng.uniform(2, 5, size=n)
    p = np.stack([np.cumsum(step * np.cos(heading)), np.cumsum(step * np.sin(heading))], axis=1)
    return np.rint(p + rng.uniform(0, 255, size=2)).astype(np.float32)


def float_stroke(rng, n):
    return rng.uniform(0, 255, size=(n, 2)).astype(np.float32)


def int_pool():
    """Smooth integer strokes of every named length and of 1 .. 40 points besides."""
    rng = np.random.RandomState(31)
    return [smooth_int_stroke(rng, n) for n in STROKE_LENGTHS + tuple(range(1, 41))]


def float_pool():
    rng = np.random.RandomState(32)
    return [float_stroke(rng, n) for n in STROKE_LENGTHS]


def short_strokes(count):
    """count strokes of 0 .. 9 integer points."""
    rng = np.random.RandomState(33)
    return [smooth_int_stroke(rng, int(rng.randint(0, 10))) for _ in range(count)]


def int_sketch(rng, lengths, pen_value=1, lift_last=True, dtype=np.int16):
    """A stroke-3 sketch of smooth integer strokes of the given lengths, the first point of each a jump from the last."""
    rows = []
    at = np.zeros(2)
    for n in lengths:
        p = smooth_int_stroke(rng, n).astype(np.float64)
        p = p - p[0] + at + np.rint(rng.uniform(-30, 30, size=2))
        d = np.diff(np.concatenate([at[None], p]), axis=0)
        pen = np.zeros((n, 1))
        pen[-1] = pen_value
        rows.append(np.concatenate([d, pen], axis=1))
        at = p[-1]
    s = np.concatenate(rows).astype(dtype)
    if not lift_last:
        s[-1, 2] = 0
    return s


def sketch_pool():
    """2 * OFFSETS_SCAN_BLOCK + 5 integer sketches: the named cases first (the first 130 hold all of them), short ones behind
    them.  Every count of the sweep takes a prefix."""
    rng = np.random.RandomState(34)
    pool = [int_sketch(rng, [40, 25, 70])]                                      # N = 1: three strokes, across a wave's width
    pool.append(int_sketch(rng, [90], lift_last=False))                        # no pen lift at all
    pool.append(int_sketch(rng, [30, 20], pen_value=2))                        # pen 2 ends no stroke: one stroke of 50 points
    pool.append(int_sketch(rng, [1, 1, 12, 1, 30, 1]))                         # one-point strokes, two of them in a row
    pool.append(int_sketch(rng, [5, LDS_POINTS + 40, 7, 3]))                   # a long stroke among short ones: beyond the LDS
    pool.append(np.zeros((0, 3), np.int16))                                    # an empty sketch
    pool.append(int_sketch(rng, [LDS_POINTS - 20, 19]))                        # LDS_POINTS - 1 rows
    pool.append(int_sketch(rng, [LDS_POINTS - 20, 20]))                        # exactly LDS_POINTS rows
    pool.append(int_sketch(rng, [LDS_POINTS - 20, 21]))                        # LDS_POINTS + 1
    pool.append(int_sketch(rng, [60, 4]))                                      # 64 rows
    pool.append(int_sketch(rng, [60, 5], lift_last=False))                     # 65 rows, the last stroke left open
    pool.append(np.array([[3, 4, 1]], np.int16))                               # one row
    pool.append(np.array([[3, 4, 0], [1, 1, 0]], np.int16))                    # two rows, no lift
    pool.append(np.zeros((9, 3), np.int16))                                    # zero offsets: every segment is degenerate
    while len(pool) < 130:
        pool.append(int_sketch(rng, [int(rng.randint(1, 60)) for _ in range(int(rng.randint(1, 7)))]))
    while len(pool) < 2 * OFFSETS_SCAN_BLOCK + 5:
        pool.append(int_sketch(rng, [int(rng.randint(1, 7)) for _ in range(int(rng.randint(1, 3)))]))
    return pool


def n_differing(a, b):
    return sum(1 for p, q in zip(a, b) if p.shape != q.shape or not np.array_equal(p.view(np.int32), q.view(np.int32)))


# ---------------------------------------------------------------- the chunk script on the golden class files
def run_chunk_script(target, *extra):
    """prep_data/prepare-distributed-quickdraw.py, in this process, on the three golden class files cut into two chunks."""
    script = os.path.join(ROOT, "prep_data", "prepare-distributed-quickdraw.py")
    inputs = os.path.join(GOLDEN, "input")
    argv = ["--dataset-dir", inputs, "--class-list", os.path.join(inputs, "classes.txt"), "--n-chunks", "2", "--n-classes", "3",
            "--target-dir", str(target)] + list(extra)
    runpy.run_path(script)["main"](argv)
