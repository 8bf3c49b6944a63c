"""Host references and fixtures shared by tests/test_preprocess_cpu.py and tests/test_gpu_preprocess.py: the host loader without
files or threads, the float64 nearest-centre rule, and the two fixtures that give the GPU tests teeth - sketches whose grid ids
depend on the summation order, and a point whose fp32 distances tie where the float64 ones do not."""
import numpy as np

from sketchformer_amd import dataloaders


# ---------------------------------------------------------------- the host pipeline
def npz_dictionary(path, centers):
    np.savez(str(path), cluster_centers=np.asarray(centers, np.float32), inertia=np.float64(0), n_iter=np.int64(1))
    return str(path)


def host_loader(name="stroke3-distributed", tokenizer=None, **over):
    """A loader object without chunk files or threads (its __init__ needs both): hparams, clamp limit and tokenizer only."""
    cls = dataloaders.get_dataloader_by_name(name)
    hps = cls.default_hparams()
    for k, v in over.items():
        hps.set_hparam(k, v)
    obj = cls.__new__(cls)
    obj.hps, obj.limit = dict(hps.values()), 1000
    if tokenizer is not None:
        obj.tokenizer = tokenizer
    return obj


def numpy_nearest(points, centers):
    """Tokenizer.nearest_center's numpy path on its own: float64 differences, squares and sum, first minimum wins."""
    p, c = np.asarray(points, np.float32).astype(np.float64), np.asarray(centers, np.float64)
    dx, dy = p[:, None, 0] - c[None, :, 0], p[:, None, 1] - c[None, :, 1]
    return (dx * dx + dy * dy).argmin(1)


def fmaf_nearest(points, centers):
    """The rule of skf_kmeans_assign_f32: dx, dy in fp32, d = fmaf(dy, dy, dx * dx) - dx * dx rounded to fp32, then dy * dy + that
    rounded once (emulated in float64: both products are exact there and the sum of two doubles rounds to fp32 once up to a
    double rounding that the fixtures stay away from)."""
    p, c = np.asarray(points, np.float32), np.asarray(centers, np.float32)
    dx, dy = p[:, None, 0] - c[None, :, 0], p[:, None, 1] - c[None, :, 1]
    xx = (dx * dx).astype(np.float32)
    d = (dy.astype(np.float64) * dy.astype(np.float64) + xx.astype(np.float64)).astype(np.float32)
    return d.argmin(1)


# ---------------------------------------------------------------- fixture (b): fp32 distances tie, float64 ones do not
def tie_fixture():
    """x = 1 + 2^-23 on the axis, centres 3 + 2^-22 and -1 + 2^-24 (all fp32 values).  Exactly, x - c0 = -(2 + 2^-23) and
    x - c1 = 2 + 2^-24; fp32 rounds both differences to magnitude 2 (the first is a tie, to even), so the fp32 distances are both 4
    and index 0 wins, while in float64 both differences are exact and centre 1 is nearer."""
    point = np.array([[1 + 2.0 ** -23, 0.0]], dtype=np.float32)
    centers = np.array([[3 + 2.0 ** -22, 0.0], [-1 + 2.0 ** -24, 0.0]], dtype=np.float32)
    return point, centers


# ---------------------------------------------------------------- fixture (a): grid ids that depend on the summation order
def block_scan_cumsum_f32(x):
    """Inclusive fp32 running sum the way a 64-lane shuffle scan computes it: per block of 64 the Hillis-Steele steps 1, 2, 4 .. 32
    (lane i adds lane i - step), then the carry of the blocks before it added to every lane."""
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    carry = np.float32(0)
    for b in range(0, len(x), 64):
        v = x[b:b + 64].copy()
        step = 1
        while step < 64:
            w = v.copy()
            w[step:] = v[step:] + v[:-step]
            v, step = w, step * 2
        v = v + carry
        out[b:b + 64] = v
        carry = v[-1]
    return out


def grid_ids(norm_xy, resolution, cumsum):
    """GridTokenizer.encode's ids of normalised fp32 offsets under the given running sum."""
    r = np.float32(resolution // 2)
    cx = np.int64((cumsum(norm_xy[:, 0]) + np.float32(1)) * r)
    cy = np.int64((cumsum(norm_xy[:, 1]) + np.float32(1)) * r)
    cx[cx == resolution] = resolution - 1
    cy[cy == resolution] = resolution - 1
    return cx + cy * resolution + 1


def normalise(sketch):
    """Offsets -> fp32 offsets divided by the larger side of the bounding box, as preprocess_per_sketch_from does."""
    from sketchformer_amd.dataloaders.distributed_stroke3 import get_bounds
    s = np.array(sketch, dtype=np.float32)
    x0, x1, y0, y1 = get_bounds(s)
    s[:, :2] /= np.float32(max([x1 - x0, y1 - y0, 1]))
    return s


def summation_order_sketches(want=8, resolution=100, tries=400):
    """Integer sketches (offsets in +-40, 20 - 200 points, a few pen lifts) from a fixed RandomState whose grid ids under the
    64-wide block scan differ from those of the sequential sum.  Returns (sketches, number searched)."""
    rng = np.random.RandomState(20240611)
    found, searched = [], 0
    while len(found) < want and searched < tries:
        searched += 1
        n = int(rng.randint(20, 201))
        s = np.zeros((n, 3), dtype=np.int16)
        s[:, :2] = rng.randint(-40, 41, size=(n, 2))
        s[rng.randint(0, n, size=3), 2] = 1
        s[-1, 2] = 1
        nrm = normalise(s)
        seq = grid_ids(nrm, resolution, lambda v: np.cumsum(v, dtype=np.float32))
        blk = grid_ids(nrm, resolution, block_scan_cumsum_f32)
        if not np.array_equal(seq, blk):
            found.append(s)
    return found, searched
