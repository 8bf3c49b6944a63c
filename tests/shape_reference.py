"""Host restatement of the shape-distance rule (include/skf.h: skf_shape_distance_f32; sketchformer_amd/csrc/skf_chamfer.hip) - the
specification the device results are compared with, bit for bit: numpy float32 with one rounding per operation (numpy fuses
nothing), an exact minimum and an exact int64 fixed-point sum.  Plus the same geometry in float64 with an ordinary mean, which the
float32 rule is held against.  A helper, not a test."""
import numpy as np

F = np.float32
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 130)          # the lengths the GPU suite draws from


def _sketch(xy, pen, dtype):
    """(points (L, 2), pen (L,) bool) of a sketch; an empty one is the single point (0, 0) with its pen lifted"""
    xy = np.asarray(xy, dtype=dtype).reshape(-1, 2)
    pen = np.asarray(pen).reshape(-1) != 0
    assert len(pen) == len(xy)
    if len(xy) == 0:
        return np.zeros((1, 2), dtype), np.ones(1, bool)
    return xy, pen


def segments(xy, pen, dtype=F):
    """-> (a (M, 2), e (M, 2), inv (M,)) of the segments: every i > 0 with pen[i - 1] == 0 joins p[i - 1] to p[i]"""
    p, pen = _sketch(xy, pen, dtype)
    idx = np.nonzero(~pen[:-1])[0] + 1
    a, e = p[idx - 1], p[idx] - p[idx - 1]
    len2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    inv = np.zeros_like(len2)
    inv[len2 > 0] = dtype(1.0) / len2[len2 > 0]
    return a, e, inv


def samples(xy, pen, S, dtype=F):
    """every point, exactly, and S - 1 interior samples a + (j / S) e of every segment"""
    p, _ = _sketch(xy, pen, dtype)
    a, e, _ = segments(xy, pen, dtype)
    out = [p]
    for j in range(1, S):
        t = dtype(j) / dtype(S)
        out.append(a + t * e)
    return np.concatenate(out, axis=0)


def nearest(s, xy, pen, dtype=F, chunk=2048):
    """d (len(s),): the distance of every sample to the nearest dot or segment of the sketch"""
    if len(s) > chunk:                                   # (a sample's minimum is its own: the table is built in slabs)
        return np.concatenate([nearest(s[at:at + chunk], xy, pen, dtype) for at in range(0, len(s), chunk)])
    p, _ = _sketch(xy, pen, dtype)
    a, e, inv = segments(xy, pen, dtype)
    qx, qy = s[:, None, 0] - p[None, :, 0], s[:, None, 1] - p[None, :, 1]
    d2 = (qx * qx + qy * qy).min(axis=1)
    if len(a):
        px, py = s[:, None, 0] - a[None, :, 0], s[:, None, 1] - a[None, :, 1]
        dot = px * e[None, :, 0] + py * e[None, :, 1]
        t = np.minimum(np.maximum(dot * inv[None, :], dtype(0)), dtype(1))
        rx, ry = px - t * e[None, :, 0], py - t * e[None, :, 1]
        d2 = np.minimum(d2, (rx * rx + ry * ry).min(axis=1))
    d = np.sqrt(d2)
    assert d.dtype == dtype
    return d


def directed(xy_a, pen_a, xy_b, pen_b, S):
    """(mean_ab, max_ab) as float32: the rule, with its fixed-point mean"""
    d = nearest(samples(xy_a, pen_a, S), xy_b, pen_b)
    q = int(np.floor(d.astype(np.float64) * 16777216.0).astype(np.int64).sum())
    mean = F((np.float64(q) / 16777216.0) / np.float64(len(d)))
    return mean, d.max()


def shape_ref(xy_a, pen_a, xy_b, pen_b, S):
    """-> float32 (4,): (mean_ab, mean_ba, max_ab, max_ba), the four outputs of a pair"""
    mab, xab = directed(xy_a, pen_a, xy_b, pen_b, S)
    mba, xba = directed(xy_b, pen_b, xy_a, pen_a, S)
    return np.array([mab, mba, xab, xba], dtype=F)


def shape_ref64(xy_a, pen_a, xy_b, pen_b, S):
    """the same geometry in float64 with an ordinary mean"""
    out = []
    for (x, p), (y, q) in (((xy_a, pen_a), (xy_b, pen_b)), ((xy_b, pen_b), (xy_a, pen_a))):
        out.append(nearest(samples(x, p, S, np.float64), y, q, np.float64))
    return np.array([out[0].mean(), out[1].mean(), out[0].max(), out[1].max()], dtype=np.float64)


def chamfer(parts):
    parts = np.asarray(parts, F)
    return F(0.5) * (parts[..., 0] + parts[..., 1])


def hausdorff(parts):
    parts = np.asarray(parts, F)
    return np.maximum(parts[..., 2], parts[..., 3])


def sample_count(pen, S):
    """n + (S - 1) * segments, or 1 for an empty sketch"""
    pen = np.asarray(pen).reshape(-1) != 0
    return 1 if len(pen) == 0 else len(pen) + (S - 1) * int((~pen[:-1]).sum())


def permute_strokes(xy, pen, order=None, rng=None):
    """the same ink with its strokes in another order (a stroke = a run of points up to and including a pen lift; the last point
    is taken as lifted)"""
    xy, pen = np.asarray(xy, F).reshape(-1, 2), (np.asarray(pen).reshape(-1) != 0).astype(np.uint8)
    pen = pen.copy()
    pen[-1] = 1
    ends = np.nonzero(pen)[0] + 1
    runs = [np.arange(s, e) for s, e in zip(np.r_[0, ends[:-1]], ends)]
    if order is None:
        order = rng.permutation(len(runs))
    idx = np.concatenate([runs[k] for k in order])
    return xy[idx], pen[idx]


def decoded_sketch(tokens, tokenizer):
    """the host decoder's drawing of a token row -> (float32 points, pen bytes); the dummy row of an empty sketch is (0, 0), lifted"""
    s3 = np.asarray(tokenizer.decode_single(np.asarray(tokens).reshape(-1)), dtype=np.float64).reshape(-1, 3)
    return np.cumsum(s3[:, :2], axis=0).astype(F), (s3[:, 2] == 1).astype(np.uint8)


def centered(xy):
    """points moved so that the centre of their bounding box is the origin, in float32 as align.sketch_chamfer(center=True) does"""
    xy = np.asarray(xy, F).reshape(-1, 2)
    if len(xy) == 0:
        return xy
    return xy - (xy.min(axis=0) + xy.max(axis=0)) * F(0.5)
