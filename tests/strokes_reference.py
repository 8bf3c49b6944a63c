"""Host restatement and fixtures shared by tests/test_strokes_cpu.py and tests/test_gpu_strokes.py.  `stroke_table` and `edit` are
the rule of include/skf.h (Stroke edits) as a per-sketch Python loop in numpy float32: positions by the sequential running sum,
one subtraction per coordinate for the first row of a selected stroke, copies and sign flips for the rest."""
import numpy as np


def absolute_f32(sketch):
    """The positions of a stroke-3 sketch: the sequential fp32 running sum of dx and of dy, one add per point, from (0, 0)."""
    s = np.asarray(sketch)[:, :2].astype(np.float32)
    out = np.empty_like(s)
    ax, ay = np.float32(0), np.float32(0)
    for j in range(len(s)):
        ax, ay = np.float32(ax + s[j, 0]), np.float32(ay + s[j, 1])
        out[j, 0], out[j, 1] = ax, ay
    return out


def stroke_ranges(sketch):
    """[(first, last)] of the strokes: maximal runs of rows that end at a row with pen == 1, or at the last row."""
    pen = np.asarray(sketch)[:, 2]
    out, first = [], 0
    for j in range(len(pen)):
        if pen[j] == 1 or j == len(pen) - 1:
            out.append((first, j))
            first = j + 1
    return out


def stroke_table(sketches):
    """list of stroke-3 arrays -> (sketch_strokes int64 (N + 1), stroke_rows int64 (T + 1), stroke_ends float32 (T, 4))"""
    sketch_strokes, stroke_rows, stroke_ends, row0 = [0], [], [], 0
    for s in sketches:
        s = np.asarray(s, np.float32).reshape(-1, 3)
        A = absolute_f32(s)
        for a, b in stroke_ranges(s):
            stroke_rows.append(row0 + a)
            stroke_ends.append([A[a, 0], A[a, 1], A[b, 0], A[b, 1]])
        row0 += len(s)
        sketch_strokes.append(len(stroke_rows))
    stroke_rows.append(row0)
    return (np.array(sketch_strokes, np.int64), np.array(stroke_rows, np.int64), np.array(stroke_ends, np.float32).reshape(-1, 4))


def edit_one(sketch, selection):
    """One output sketch: `selection` over the strokes of `sketch` (k >= 0 forwards, ~k backwards, anything else absent);
    sketch=None stands for a source outside the batch.  -> float32 (n', 3)"""
    if sketch is None:
        return np.zeros((0, 3), np.float32)
    s = np.asarray(sketch, np.float32).reshape(-1, 3)
    A = absolute_f32(s)
    ranges = stroke_ranges(s)
    rows = []
    E = np.zeros(2, np.float32)
    for k in selection:
        k = int(k)
        back = k < 0
        kk = ~k if back else k
        if kk >= len(ranges):
            continue
        a, b = ranges[kk]
        if back:
            part = np.empty((b - a + 1, 3), np.float32)
            part[0, :2] = A[b] - E
            part[1:, :2] = -s[a + 1:b + 1, :2][::-1]
            E = A[a]
        else:
            part = s[a:b + 1].copy()
            part[0, :2] = A[a] - E
            E = A[b]
        part[:, 2] = 0
        part[-1, 2] = 1
        assert part.dtype == np.float32
        rows.append(part)
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), np.float32)


def edit(sketches, src, selections):
    """The M output sketches of an edit: src[m] names the source (outside [0, N): no rows), selections[m] its list."""
    N = len(sketches)
    return [edit_one(sketches[int(s)] if 0 <= int(s) < N else None, sel) for s, sel in zip(src, selections)]


def pack(sketches):
    """list of (n, 3) arrays -> (flat float32 (P, 3), offsets int64 (N + 1))"""
    lens = np.array([len(s) for s in sketches], np.int64)
    offsets = np.zeros(len(sketches) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    parts = [np.asarray(s, np.float32).reshape(-1, 3) for s in sketches if len(s)]
    flat = np.ascontiguousarray(np.concatenate(parts, axis=0)) if parts else np.zeros((0, 3), np.float32)
    return flat, offsets


def pack_lists(lists):
    """list of selection lists -> (sel int32 (Q,), sel_offsets int64 (M + 1))"""
    lens = np.array([len(l) for l in lists], np.int64)
    sel_offsets = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=sel_offsets[1:])
    sel = np.array([int(k) for l in lists for k in l], np.int32)
    return sel, sel_offsets


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- fixtures
def int_sketch(rng, lengths, lift_last=True):
    """A stroke-3 sketch of integer offsets with strokes of the given lengths; positions stay far below 2^24."""
    rows = []
    for n in lengths:
        part = np.zeros((n, 3), np.float32)
        part[:, :2] = rng.randint(-9, 10, size=(n, 2))
        part[0, :2] = rng.randint(-40, 41, size=2)
        part[-1, 2] = 1
        rows.append(part)
    s = np.concatenate(rows, axis=0)
    if not lift_last:
        s[-1, 2] = 0
    return s


def table_batch():
    """The batch of the table and edit tests: strokes of 1, 2, 63, 64, 65 and 130 rows; a sketch of one stroke; a sketch of 65
    one-row strokes; an unterminated last stroke; empty sketches first, in the middle and last; non-integer values, zero offsets
    and a stored -0.0; a sketch beyond the on-chip length."""
    rng = np.random.RandomState(51)
    batch = [np.zeros((0, 3), np.float32)]
    batch.append(int_sketch(rng, [1, 2, 63, 64, 65, 130]))
    batch.append(int_sketch(rng, [17]))
    s = int_sketch(rng, [1] * 65)
    batch.append(s)
    batch.append(int_sketch(rng, [5, 9], lift_last=False))
    batch.append(np.zeros((0, 3), np.float32))
    f = int_sketch(rng, [7, 64, 3, 70])
    f[:, :2] = (rng.normal(size=f[:, :2].shape) * 37.3).astype(np.float32)
    f[3, :2] = 0.0
    f[7, 0] = -0.0                                                               # the first row of the second stroke
    f[9, 1] = -0.0
    f[20, :2] = (0.0, -0.0)
    batch.append(f)
    batch.append(int_sketch(rng, [300, 250, 40]))                               # 590 rows: its positions go through the workspace
    g = int_sketch(rng, [4, 4])
    g[:, 2] = (0, 2, 0, 0, 0, 0, 0, 0)                                           # pen 2 ends no stroke: one stroke, never lifted
    batch.append(g)
    batch.append(np.zeros((0, 3), np.float32))
    return batch


def edit_cases(batch):
    """(src, selections) over table_batch(): lists of 0, 1, 64, 65 and 129 entries, mixed directions, a stroke listed twice, M > N,
    src not monotonic, absent entries at the start, in the middle and at the end of a list."""
    rng = np.random.RandomState(52)
    counts = [len(stroke_ranges(np.asarray(s).reshape(-1, 3))) for s in batch]
    N = len(batch)
    src, lists = [], []

    def add(s, l):
        src.append(s)
        lists.append([int(k) for k in l])

    def draw(s, n):
        k = rng.randint(0, counts[s], size=n)
        return np.where(rng.rand(n) < 0.5, k, ~k)
    add(1, [])                                                                  # an empty list
    add(3, draw(3, 64))
    add(1, [2])
    add(3, draw(3, 65))
    add(3, draw(3, 129))
    add(1, [5, ~5, 0, ~1, 2, 2, ~3, 4])                                         # a stroke twice, both directions
    add(6, [counts[6], 0, ~1, counts[6] + 3, ~(counts[6]), 2, ~3, counts[6]])   # absent: first, middle, last
    add(-1, [0, 1])                                                             # no such sketch
    add(N, [0, ~0])
    add(0, [0, ~0])                                                             # an empty source: no stroke to name
    add(7, [~2, ~1, ~0])                                                        # drawn backwards in time
    add(7, [0, 1, 2])                                                           # the identity
    add(4, [1, 0])                                                              # the unterminated stroke first
    add(8, [0, ~0, 1])
    add(2, [~0])
    for s in range(N):                                                          # the identity of everything: M > N
        add(s, range(counts[s]))
    return src, lists


def ink_fixture():
    """Integer sketches of 3 - 5 strokes with distinct ink, for the order-blindness checks -> (sketches, orders): orders[i] is a
    non-identity permutation of sketch i's strokes."""
    rng = np.random.RandomState(53)
    sketches, orders = [], []
    for i in range(6):
        n = 3 + i % 3
        sketches.append(int_sketch(rng, [int(v) for v in rng.randint(2, 9, size=n)]))
        p = np.roll(np.arange(n), 1 + i % (n - 1))
        orders.append([int(k) for k in p])
    return sketches, orders
