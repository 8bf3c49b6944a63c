"""The token dictionary as a product of this repository: Lloyd k-means on the device for 2-D points (ops.kmeans_step /
ops.kmeans_assign over skf_kmeans.hip), the initialisations on the host, and the two dictionary file formats.

What prep_data/sketch_token/create_token_dict.py:104-109 of the reference asks of sklearn - KMeans(n_clusters=1000, n_init=10,
max_iter=500, tol=1e-6).fit(points) - is `fit` here.  Differences, all deliberate: the initialisation does not follow sklearn's
random stream (see `init_centers`), a centre that loses all its points keeps its coordinates (sklearn relocates it), and the
arithmetic is the device's: bit-identical from run to run.
"""
import os

import numpy as np

KMEANSPP_SUBSAMPLE = 64          # k-means++ looks at no more than this many points per centre


class KMeansResult(object):
    """cluster_centers_ (K, 2) float32, inertia_, n_iter_, n_empty_ of the winning run, labels_ (N,) int32 or None, and
    runs_: per run dict(inertia, n_iter, n_empty, converged, init_centers) in the order they ran."""

    def __init__(self, cluster_centers_, inertia_, n_iter_, n_empty_, labels_, runs_):
        self.cluster_centers_ = cluster_centers_
        self.inertia_ = inertia_
        self.n_iter_ = n_iter_
        self.n_empty_ = n_empty_
        self.labels_ = labels_
        self.runs_ = runs_
        self.n_features_in_ = 2


def _rows(points, idx):
    """points[idx] as a float32 numpy array, for a numpy array or a (device) tensor."""
    if isinstance(points, np.ndarray):
        return np.asarray(points[idx], dtype=np.float32)
    import torch
    return points[torch.as_tensor(idx, dtype=torch.int64, device=points.device)].to(torch.float32).cpu().numpy()


def kmeanspp_indices(sub, n_clusters, rng):
    """D^2 sampling (Arthur & Vassilvitskii 2007) over the rows of `sub` (M, 2): the first centre uniformly, every next one with
    probability proportional to its squared distance to the nearest centre chosen so far.  -> n_clusters distinct row indices.
    Rows at distance zero (chosen ones, and their duplicates) are never drawn while any other remains; when none remains the
    rest is drawn uniformly from the rows not chosen yet."""
    sub = np.asarray(sub, dtype=np.float64)
    M = sub.shape[0]
    if n_clusters > M:
        raise ValueError("n_clusters = %d exceeds the %d points to choose from" % (n_clusters, M))
    chosen = np.empty(n_clusters, dtype=np.int64)
    taken = np.zeros(M, dtype=bool)
    chosen[0] = rng.randint(M)
    taken[chosen[0]] = True
    d2 = ((sub - sub[chosen[0]]) ** 2).sum(1)
    for c in range(1, n_clusters):
        d2[taken] = 0.0
        total = d2.sum()
        if total > 0.0:
            # first row whose running sum exceeds the draw: its own weight is positive, so it is neither chosen nor a duplicate
            i = int(np.searchsorted(np.cumsum(d2), rng.random_sample() * total, side="right"))
            if i >= M:                               # the draw rounded up to the total
                i = int(np.nonzero(d2 > 0.0)[0][-1])
        else:
            free = np.nonzero(~taken)[0]
            i = int(free[rng.randint(len(free))])
        chosen[c] = i
        taken[i] = True
        d2 = np.minimum(d2, ((sub - sub[i]) ** 2).sum(1))
    return chosen


def init_centers(points, n_clusters, init="k-means++", seed=0):
    """Initial centres (n_clusters, 2) float32 for `points` (N, 2), a numpy array or a tensor.
    'k-means++': D^2 sampling in numpy over a seeded subsample of at most 64 * n_clusters points (kmeanspp_indices).  This is
        NOT sklearn's random stream, nor its greedy variant with several trials per centre: the same seed gives other centres
        than sklearn's, and a dictionary fitted here is not reproducible by sklearn (nor the reverse).
    'random': n_clusters distinct points, seeded.
    Both are reproducible: the same points, n_clusters, init and seed give the same rows."""
    N = int(points.shape[0])
    if n_clusters > N:
        raise ValueError("n_clusters = %d exceeds the number of points %d" % (n_clusters, N))
    rng = np.random.RandomState(seed)
    if init == "random":
        return _rows(points, rng.choice(N, n_clusters, replace=False))
    if init == "k-means++":
        m = min(N, KMEANSPP_SUBSAMPLE * n_clusters)
        pick = np.sort(rng.choice(N, m, replace=False)) if m < N else np.arange(N)
        sub = _rows(points, pick)
        return sub[kmeanspp_indices(sub, n_clusters, rng)]
    raise ValueError("init must be 'k-means++', 'random' or a (K, 2) array (got %r)" % (init,))


def fit(points, n_clusters, n_init=10, max_iter=500, tol=1e-6, init="k-means++", seed=0, check_every=8, return_labels=True):
    """Lloyd k-means of `points` (N, 2; a device tensor or a numpy array) into n_clusters centres on the GPU -> KMeansResult.

    tol has sklearn's meaning: a run stops after the iteration whose squared centre shift sum |c_new - c_old|^2 is at most
    tol * mean(var(points, axis=0)).  The stop flag lives on the device: iterations are enqueued check_every at a time and the
    flag is read once per group, never per iteration; n_iter_ is the iteration that set it (max_iter when none did), and centres,
    labels and inertia are that iteration's.  init: 'k-means++' | 'random' (init_centers; run r uses seed + r) or a (K, 2) array
    (one run).  With n_init > 1 the run with the lowest inertia wins, the earlier one on equal inertia.  Two fits with the same
    arguments return bit-equal centres.  return_labels=False leaves labels_ None (20 MB at 5 M points)."""
    import torch
    from . import ops
    if isinstance(points, np.ndarray):
        pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).cuda()
    else:
        pts = points.to(torch.float32)
        if not pts.is_cuda:
            pts = pts.cuda()
    if pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError("points must be (N, 2)")
    if pts.stride(1) != 1 or pts.stride(0) % 2 or pts.data_ptr() % 8:
        pts = pts.contiguous()
    N, K = pts.shape[0], int(n_clusters)
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("points must be finite")
    given = not isinstance(init, str)
    if given:
        init = np.asarray(init, dtype=np.float32)
        if init.shape != (K, 2):
            raise ValueError("an init array must have shape (n_clusters, 2) = (%d, 2), got %r" % (K, init.shape))
        n_init = 1
    if max_iter < 1 or n_init < 1 or check_every < 1:
        raise ValueError("max_iter, n_init and check_every must be at least 1")
    tol_abs = float(tol) * float(pts.to(torch.float64).var(dim=0, unbiased=False).mean())
    scale_exp = ops.kmeans_scale_exp(float(pts.abs().max()))
    labels = torch.empty(N, dtype=torch.int32, device=pts.device)
    counts = torch.empty(K, dtype=torch.int32, device=pts.device)
    ws = torch.empty(max(int(ops._lib.load().skf_kmeans_workspace_bytes(N, K)), 256), dtype=torch.uint8, device=pts.device)
    best, runs = None, []
    for r in range(n_init):
        c0 = init if given else init_centers(pts, K, init, seed + r)
        centers = torch.from_numpy(np.ascontiguousarray(c0)).to(pts.device)
        state = ops.new_kmeans_state(pts.device)
        done = 0
        while True:
            group = min(check_every, max_iter - done)
            for _ in range(group):
                ops.kmeans_step(pts, centers, state, scale_exp, tol_abs, labels=labels, counts=counts, workspace=ws)
            done += group
            st = ops.read_kmeans_state(state)            # the one host read of the group
            if st["converged"] or done >= max_iter:
                break
        run = {"inertia": st["inertia"], "n_iter": st["iterations"], "n_empty": st["n_empty"], "converged": st["converged"],
               "init_centers": np.array(c0, dtype=np.float32)}
        runs.append(run)
        if best is None or run["inertia"] < best[0]["inertia"]:
            best = (run, centers.cpu().numpy(), labels.cpu().numpy() if return_labels else None)
    run, c, lab = best
    return KMeansResult(c, run["inertia"], run["n_iter"], run["n_empty"], lab, runs)


def save_dictionary(path, result):
    """Write a fitted dictionary.  `.npz`: cluster_centers (float32), inertia, n_iter - read back with nothing but numpy
    (load_centers, Tokenizer).  `.pkl` (any other extension): a pickled sklearn.cluster.KMeans that carries the fitted centres -
    the file the reference's utils/tokenizer.py:24 unpickles and calls predict on; needs sklearn to write and to read."""
    centers = np.ascontiguousarray(result.cluster_centers_, dtype=np.float32)
    if centers.ndim != 2 or centers.shape[1] != 2:
        raise ValueError("cluster_centers_ must be (K, 2)")
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    if path.endswith(".npz"):
        with open(path, "wb") as f:
            np.savez(f, cluster_centers=centers, inertia=np.float64(result.inertia_), n_iter=np.int64(result.n_iter_))
        return path
    try:
        from sklearn.cluster import KMeans
    except ImportError as e:
        raise ImportError("writing a pickled dictionary (%s) needs scikit-learn: %s.  Save to a path ending in .npz instead: "
                          "Tokenizer reads it with numpy alone" % (path, e))
    import pickle
    km = KMeans(n_clusters=centers.shape[0], n_init=1)
    km.cluster_centers_ = centers
    km.inertia_ = float(result.inertia_)
    km.n_iter_ = int(result.n_iter_)
    km.n_features_in_ = 2
    km._n_threads = 1                                    # what fit() leaves behind and predict() reads
    labels = getattr(result, "labels_", None)
    if labels is not None:
        km.labels_ = np.asarray(labels, dtype=np.int32)
    with open(path, "wb") as f:
        pickle.dump(km, f)
    return path


def load_centers(path):
    """The (K, 2) float32 centres of a dictionary file: `.npz` with numpy alone, anything else through pickle (sklearn)."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            centers = np.asarray(z["cluster_centers"], dtype=np.float32)
    else:
        import pickle
        with open(path, "rb") as f:
            centers = np.asarray(pickle.load(f).cluster_centers_, dtype=np.float32)
    if centers.ndim != 2 or centers.shape[1] != 2:
        raise ValueError("%s: cluster_centers must be (K, 2), got %r" % (path, centers.shape))
    return centers
