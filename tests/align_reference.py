"""Host restatements of the sequence-alignment kernels (sketchformer_amd/csrc/skf_align.hip) - the specification the device
results are compared with, exactly: the unit-cost Levenshtein distance as a plain integer dynamic program, dynamic time warping in
numpy float32 with one rounding per operation, and the rule that cuts the content out of a token row.  A helper, not a test."""
import numpy as np

# the lengths both suites walk: empty, the shortest rows, the edges of a 64-lane wave and of its multiples, a typical sketch, the limit
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 511, 512)
WIDTHS = (64, 128, 256, 512)                       # one per strip width S = 1, 2, 4, 8 of the kernel


def edit_distance_ref(a, b):
    """Levenshtein distance between two sequences of integers: insert, delete, substitute cost 1 each."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    prev = list(range(len(b) + 1))                 # D(0, j) = j
    for i, x in enumerate(a, 1):
        left = i                                   # D(i, 0) = i
        cur = [left]
        for j, y in enumerate(b):
            v = prev[j] if x == y else prev[j] + 1
            up = prev[j + 1] + 1
            if up < v:
                v = up
            if left + 1 < v:
                v = left + 1
            cur.append(v)
            left = v
        prev = cur
    return prev[-1]


def _points(p):
    p = np.asarray(p, dtype=np.float32).reshape(-1, 2)
    return p if len(p) else np.zeros((1, 2), dtype=np.float32)          # an empty side: the single point (0, 0)


def local_cost(a, b):
    """c(i, j) = sqrt(dx * dx + dy * dy) in float32, every operation rounded on its own (numpy fuses nothing)"""
    a, b = _points(a), _points(b)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    c = np.sqrt(dx * dx + dy * dy)
    assert c.dtype == np.float32
    return c


def dtw_ref_cells(a, b):
    """DTW cell by cell, row-major: D(0, 0) = c(0, 0), the borders are running sums,
    D(i, j) = c(i, j) + min(D(i-1, j), D(i, j-1), D(i-1, j-1)), all float32.  -> the float32 D(na - 1, nb - 1)"""
    c = local_cost(a, b)
    D = np.empty_like(c)
    for i in range(c.shape[0]):
        for j in range(c.shape[1]):
            if i == 0 and j == 0:
                D[i, j] = c[i, j]
            elif i == 0:
                D[i, j] = c[i, j] + D[i, j - 1]
            elif j == 0:
                D[i, j] = c[i, j] + D[i - 1, j]
            else:
                D[i, j] = c[i, j] + min(D[i - 1, j], D[i, j - 1], D[i - 1, j - 1])
    return D[-1, -1]


def dtw_ref(a, b):
    """The same recurrence swept along anti-diagonals (whole diagonals as float32 vectors): every cell is the same float32
    expression of its three neighbours and min is exact, so the sweep order cannot change a bit (tests/test_align_cpu.py compares
    the two).  -> the float32 D(na - 1, nb - 1)"""
    c = local_cost(a, b)
    na, nb = c.shape
    inf = np.float32(np.inf)
    D = np.full((na + 1, nb + 1), inf, dtype=np.float32)               # row 0 and column 0: outside the table
    D[0, 0] = 0.0
    for k in range(na + nb - 1):                                         # cells (i, k - i)
        i = np.arange(max(0, k - nb + 1), min(na, k + 1))
        j = k - i
        best = np.minimum(np.minimum(D[i, j + 1], D[i + 1, j]), D[i, j])
        D[i + 1, j + 1] = c[i, j] + best
    assert D.dtype == np.float32
    return D[na, nb]


def token_span_ref(row, tokenizer):
    """The content of a token row: what lies behind one leading SOS, if present, and in front of the first EOS or PAD (or the
    row's end).  -> a list of ints"""
    row = [int(t) for t in np.asarray(row).reshape(-1)]
    if row and row[0] == tokenizer.SOS:
        row = row[1:]
    out = []
    for t in row:
        if t == tokenizer.EOS or t == tokenizer.PAD:
            break
        out.append(t)
    return out


def decoded_points(tokens, tokenizer):
    """The host decoder's drawing of a token row as absolute float32 positions (the dummy row of an empty sketch is (0, 0))"""
    s3 = np.asarray(tokenizer.decode_single(np.asarray(tokens).reshape(-1)), dtype=np.float64).reshape(-1, 3)
    return np.cumsum(s3[:, :2], axis=0).astype(np.float32)


def length_pairs(T):
    """every (la, lb) of LENGTHS^2 that fits rows of width T"""
    fit = [n for n in LENGTHS if n <= T]
    return [(la, lb) for la in fit for lb in fit]
