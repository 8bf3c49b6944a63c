"""Device k-means (skf_kmeans_assign_f32 / skf_kmeans_step_f32 through ops.kmeans_assign, ops.kmeans_step and kmeans.fit) against a
float64 numpy oracle written here: D = (x - cx)^2 + (y - cy)^2 on the float32 inputs, argmin with the first minimum winning."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEAR_TIE = 1.0 + 2.0 ** -20      # each fp32 distance is within (1 +- 2^-22) of the exact one: a label may differ from the oracle's
                                 # argmin only where its exact distance is within this factor of the minimum


def _D(p, c):
    p64, c64 = p.astype(np.float64), c.astype(np.float64)
    dx, dy = p64[:, None, 0] - c64[None, :, 0], p64[:, None, 1] - c64[None, :, 1]
    return dx * dx + dy * dy


def _dev(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assign(p, c, dist=True):
    from sketchformer_amd import ops
    out = ops.kmeans_assign(_dev(p), _dev(c), return_dist=dist)
    torch.cuda.synchronize()
    if dist:
        assert out[0].dtype == torch.int32 and out[1].dtype == torch.float32 and out[0].shape == out[1].shape == (len(p),)
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def _step(p, c, tol_abs=-1.0, state=None):
    """One ops.kmeans_step on copies -> (labels, counts, new centres, state dict)"""
    from sketchformer_amd import ops
    tp, tc = _dev(p), _dev(c).clone()
    state = ops.new_kmeans_state(tp.device) if state is None else state
    e = ops.kmeans_scale_exp(float(np.abs(p).max()))
    labels, counts = ops.kmeans_step(tp, tc, state, e, tol_abs)
    st = ops.read_kmeans_state(state)
    return labels.cpu().numpy(), counts.cpu().numpy(), tc.cpu().numpy(), st


def _check_labels(D, labels):
    """rule 3: the exact distance of the device's choice is within NEAR_TIE of the minimum; -> rows that differ from the argmin"""
    rows = np.arange(len(D))
    assert labels.min() >= 0 and labels.max() < D.shape[1]
    assert (D[rows, labels] <= D.min(1) * NEAR_TIE).all()
    return int((labels != D.argmin(1)).sum())


# ------------------------------------------------------------------ exact lattice
@pytest.fixture(scope="module")
def lattice():
    rs = np.random.RandomState(0)
    p = (rs.randint(-64, 65, size=(4099, 2)) / 64.0).astype(np.float32)
    c = (rs.randint(-64, 65, size=(257, 2)) / 64.0).astype(np.float32)
    D = _D(p, c)
    # every difference, square and sum is exact in fp32: multiples of 2^-12 below 2^4
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D) and np.array_equal(D * 4096, np.round(D * 4096))
    want = D.argmin(1)
    ties = int(((D == D.min(1, keepdims=True)).sum(1) > 1).sum())
    dups = len(c) - len(np.unique(c, axis=0))
    empty = len(c) - len(np.unique(want))
    assert ties >= 1 and dups >= 1 and empty >= 1, (ties, dups, empty)
    D.setflags(write=False)
    return p, c, D, want


def test_lattice_assign_is_exact(lattice):
    """No tolerance: labels equal the first-minimum argmin (exact ties, duplicate centres), distances equal bit for bit; the same
    through views with a larger row pitch."""
    p, c, D, want = lattice
    labels, dist = _assign(p, c)
    assert np.array_equal(labels, want.astype(np.int32)), "%d labels differ" % (labels != want).sum()
    assert np.array_equal(dist.view(np.uint32), D.min(1).astype(np.float32).view(np.uint32))
    assert np.array_equal(_assign(p, c, dist=False), labels)
    wp = torch.full((len(p), 6), 7.0, device="cuda"); wp[:, 2:4] = _dev(p)
    wc = torch.full((len(c), 4), -3.0, device="cuda"); wc[:, :2] = _dev(c)
    l2, d2 = _assign(wp[:, 2:4], wc[:, :2])
    assert np.array_equal(l2, labels) and np.array_equal(d2.view(np.uint32), dist.view(np.uint32))


def test_lattice_assign_smallest_and_largest_k(lattice):
    p, c, D, want = lattice
    labels, dist = _assign(p[:1], c[:1])                                 # N = 1, K = 1
    assert labels.tolist() == [0] and dist[0] == np.float32(D[0, 0])
    rs = np.random.RandomState(1)
    big = (rs.randint(-64, 65, size=(4096, 2)) / 64.0).astype(np.float32)    # K = 4096: every lattice value many times over
    Db = _D(p, big)
    labels, dist = _assign(p, big)
    assert np.array_equal(labels, Db.argmin(1).astype(np.int32))
    assert np.array_equal(dist.view(np.uint32), Db.min(1).astype(np.float32).view(np.uint32))


def _oracle_step(p, c, labels):
    K = len(c)
    n = np.bincount(labels, minlength=K)
    sx = np.bincount(labels, weights=p[:, 0].astype(np.float64), minlength=K)
    sy = np.bincount(labels, weights=p[:, 1].astype(np.float64), minlength=K)
    new = c.copy()
    live = n > 0
    new[live, 0] = (sx[live] / n[live]).astype(np.float32)
    new[live, 1] = (sy[live] / n[live]).astype(np.float32)
    shift = ((new.astype(np.float64) - c.astype(np.float64)) ** 2).sum()
    return n, new, shift


def test_lattice_one_step_is_exact(lattice):
    """Counts equal, new centres bit-equal to float32(sum / n) (the sums of lattice values are exact in float64 and in the integer
    accumulators), empty centres untouched, the inertia - multiples of 2^-12 summing below 2^24 - equal exactly."""
    p, c, D, want = lattice
    labels, counts, new, st = _step(p, c)
    n, wnew, wshift = _oracle_step(p, c, want)
    assert np.array_equal(labels, want.astype(np.int32)) and np.array_equal(counts, n.astype(np.int32))
    assert np.array_equal(new.view(np.uint32), wnew.view(np.uint32))
    assert np.array_equal(new[n == 0], c[n == 0]) and st["n_empty"] == int((n == 0).sum()) >= 1
    inertia = D.min(1).sum()
    assert inertia * 4096 < 2 ** 24 and st["inertia"] == inertia
    assert abs(st["shift"] - wshift) <= 1e-6 * wshift
    assert st["iterations"] == 1 and not st["converged"]


def test_lattice_one_step_largest_k(lattice):
    """K = 4096: the accumulating kernel's largest LDS image (centres + sums + counts)."""
    p = lattice[0]
    rs = np.random.RandomState(1)
    big = (rs.randint(-64, 65, size=(4096, 2)) / 64.0).astype(np.float32)
    want = _D(p, big).argmin(1)
    labels, counts, new, st = _step(p, big)
    n, wnew, _ = _oracle_step(p, big, want)
    assert np.array_equal(labels, want.astype(np.int32)) and np.array_equal(counts, n.astype(np.int32))
    assert np.array_equal(new.view(np.uint32), wnew.view(np.uint32)) and st["n_empty"] == int((n == 0).sum())


# ------------------------------------------------------------------ random floats
@pytest.fixture(scope="module")
def floats():
    rs = np.random.RandomState(2)
    p = rs.normal(0, 0.08, size=(20000, 2)).astype(np.float32)
    c = rs.normal(0, 0.08, size=(1000, 2)).astype(np.float32)
    return p, c


def test_float_assign_within_near_tie_rule(floats):
    """Every device label is a minimum up to (1 + 2^-20); at most 0.1 % of the rows may differ from the oracle's argmin at all (a
    condition, not a measurement: fp32 emulation of the definition on the CPU differs in 0 rows of this input)."""
    p, c = floats
    D = _D(p, c)
    labels, dist = _assign(p, c)
    differ = _check_labels(D, labels)
    print("rows that differ from the float64 argmin: %d of %d" % (differ, len(p)))
    assert differ <= len(p) // 1000
    rows = np.arange(len(p))
    assert (np.abs(dist - D[rows, labels]) <= D[rows, labels] * 2.0 ** -22).all()


def test_float_ten_steps(floats):
    """Ten Lloyd steps from a given init, each checked on the device's own centres going in and labels coming out: labels by the
    near-tie rule; every new centre within 2^-22 max|coordinate| of the float64 mean of its labelled points (quantisation <= 2^-30
    of the maximum, final rounding <= 2^-24 of the value); inertia within 2e-6 relative of the float64 sum of the chosen distances
    (per-term error <= 2^-22 on non-negative terms, an eightfold margin); the inertia sequence never increases."""
    from sketchformer_amd import ops
    p, c = floats
    tp, tc = _dev(p), _dev(c).clone()
    state = ops.new_kmeans_state(tp.device)
    e = ops.kmeans_scale_exp(float(np.abs(p).max()))
    amax = float(np.abs(p).max())
    rows = np.arange(len(p))
    inertias = []
    for it in range(10):
        before = tc.cpu().numpy()
        labels, counts = ops.kmeans_step(tp, tc, state, e, -1.0)
        st = ops.read_kmeans_state(state)
        labels, counts, after = labels.cpu().numpy(), counts.cpu().numpy(), tc.cpu().numpy()
        D = _D(p, before)
        _check_labels(D, labels)
        n = np.bincount(labels, minlength=len(c))
        assert np.array_equal(counts, n.astype(np.int32)) and st["n_empty"] == int((n == 0).sum()) and st["iterations"] == it + 1
        live = n > 0
        mean = np.stack([np.bincount(labels, weights=p[:, a].astype(np.float64), minlength=len(c)) for a in (0, 1)], 1)[live] / n[live, None]
        err = np.abs(after[live].astype(np.float64) - mean).max()
        assert err <= 2.0 ** -22 * amax, err
        assert np.array_equal(after[~live], before[~live])
        want = D[rows, labels].sum()
        rel = abs(st["inertia"] - want) / want
        print("step %d: inertia %.9g, rel. error %.3g, centre error %.3g (bound %.3g)" % (it, st["inertia"], rel, err, 2.0 ** -22 * amax))
        assert rel <= 2e-6
        inertias.append(st["inertia"])
    assert all(b <= a for a, b in zip(inertias, inertias[1:])), inertias


# ------------------------------------------------------------------ the fit loop
def _blobs(seed, n, k, spread=0.01):
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-1, 1, size=(k, 2))
    return (centres[rs.randint(0, k, n)] + spread * rs.normal(size=(n, 2))).astype(np.float32)


def _same(a, b):
    return (np.array_equal(a.cluster_centers_.view(np.uint32), b.cluster_centers_.view(np.uint32)) and np.array_equal(a.labels_, b.labels_)
            and a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_ and a.n_empty_ == b.n_empty_)


def test_fit_is_deterministic(floats):
    from sketchformer_amd import kmeans
    p = floats[0]
    kw = dict(n_init=2, max_iter=40, init="k-means++", seed=5)
    a = kmeans.fit(p, 100, **kw)
    b = kmeans.fit(torch.from_numpy(p).cuda(), 100, **kw)
    c = kmeans.fit(p, 100, check_every=3, **kw)
    assert a.cluster_centers_.dtype == np.float32 and a.cluster_centers_.shape == (100, 2) and a.labels_.shape == (len(p),)
    assert _same(a, b) and _same(a, c)
    assert [r["inertia"] for r in a.runs_] == [r["inertia"] for r in c.runs_]


def test_stop_flag():
    from sketchformer_amd import kmeans, ops
    p = _blobs(3, 4000, 8)
    full = kmeans.fit(p, 8, n_init=1, max_iter=100, init="random", seed=1)
    assert 1 <= full.n_iter_ < 100 and full.runs_[0]["converged"]
    short = kmeans.fit(p, 8, n_init=1, max_iter=full.n_iter_, init="random", seed=1)
    assert short.n_iter_ == full.n_iter_ and _same(full, short)
    # by hand: step until the flag is up, then one more group of eight changes nothing
    tp = _dev(p)
    tc = _dev(full.runs_[0]["init_centers"]).clone()
    state = ops.new_kmeans_state(tp.device)
    e = ops.kmeans_scale_exp(float(np.abs(p).max()))
    tol_abs = 1e-6 * float(p.astype(np.float64).var(0).mean())
    labels = torch.empty(len(p), dtype=torch.int32, device="cuda")
    counts = torch.empty(8, dtype=torch.int32, device="cuda")
    for _ in range(full.n_iter_):
        ops.kmeans_step(tp, tc, state, e, tol_abs, labels=labels, counts=counts)
    st = ops.read_kmeans_state(state)
    assert st["converged"] and st["iterations"] == full.n_iter_ and st["shift"] <= tol_abs and st["inertia"] == full.inertia_
    snap = (tc.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy())
    assert np.array_equal(snap[0], full.cluster_centers_) and np.array_equal(snap[1], full.labels_)
    for _ in range(8):
        ops.kmeans_step(tp, tc, state, e, tol_abs, labels=labels, counts=counts)
    assert ops.read_kmeans_state(state) == st
    assert all(np.array_equal(a, b) for a, b in zip(snap, (tc.cpu().numpy(), labels.cpu().numpy(), counts.cpu().numpy())))
    # max_iter below convergence: the loop stops there, whatever the group size
    q = np.random.RandomState(4).normal(0, 0.08, size=(5000, 2)).astype(np.float32)
    r = kmeans.fit(q, 100, n_init=1, max_iter=3, init="random", seed=0)
    assert r.n_iter_ == 3 and not r.runs_[0]["converged"]


def _lloyd64(p, c0, max_iter=300):
    p64, c = p.astype(np.float64), c0.astype(np.float64).copy()
    labels = None
    for _ in range(max_iter):
        D = (p64[:, None, 0] - c[None, :, 0]) ** 2 + (p64[:, None, 1] - c[None, :, 1]) ** 2
        new = D.argmin(1)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        n = np.bincount(labels, minlength=len(c))
        for a in (0, 1):
            s = np.bincount(labels, weights=p64[:, a], minlength=len(c))
            c[n > 0, a] = s[n > 0] / n[n > 0]
    return D.min(1).sum()


@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_fit_end_to_end(init):
    """30000 points from 64 blobs, n_init = 3: the chosen run has the lowest of the three inertias (the earliest on a tie), and it is
    no worse than 1.05 x what float64 Lloyd in numpy reaches from the SAME initial centres - same init, same algorithm: the margin
    only absorbs near-tie label flips and the tol stop.  Ratio observed on an MI355X: 1.000013 (k-means++, 40 iterations) and
    1.000010 (random, 27 iterations)."""
    from sketchformer_amd import kmeans
    p = _blobs(7, 30000, 64, spread=0.03)
    r = kmeans.fit(p, 64, n_init=3, init=init, seed=11)
    inertias = [run["inertia"] for run in r.runs_]
    assert len(inertias) == 3 and r.inertia_ == min(inertias)
    win = inertias.index(min(inertias))
    assert r.n_iter_ == r.runs_[win]["n_iter"] and r.cluster_centers_.shape == (64, 2)
    assert len({run["init_centers"].tobytes() for run in r.runs_}) == 3          # three different starts
    D = _D(p, r.cluster_centers_)
    assert r.labels_.shape == (30000,) and r.labels_.dtype == np.int32
    want = _lloyd64(p, r.runs_[win]["init_centers"])
    print("fit %s: inertia %.9g, float64 Lloyd from the same init %.9g, ratio %.6f, n_iter %d" % (init, r.inertia_, want, r.inertia_ / want, r.n_iter_))
    assert r.inertia_ <= 1.05 * want
    assert abs(D.min(1).sum() - r.inertia_) <= 0.05 * r.inertia_               # the reported centres are the ones the inertia belongs to


# ------------------------------------------------------------------ files and the tokenizer
def _sketches():
    rs = np.random.RandomState(9)
    out = []
    for _ in range(5):
        n = rs.randint(8, 20)
        s = np.zeros((n, 3), dtype=np.float32)
        s[:, :2] = rs.normal(0, 0.08, size=(n, 2))
        s[rs.choice(n - 1, 2, replace=False), 2] = 1
        s[-1, 2] = 1
        out.append(s)
    return out


@pytest.fixture(scope="module")
def small_fit():
    from sketchformer_amd import kmeans
    p = np.random.RandomState(8).normal(0, 0.08, size=(6000, 2)).astype(np.float32)
    return kmeans.fit(p, 50, n_init=1, max_iter=30, seed=2)


def _round_trip(path, small_fit):
    from sketchformer_amd import kmeans
    from sketchformer_amd.utils import Tokenizer
    kmeans.save_dictionary(path, small_fit)
    assert np.array_equal(kmeans.load_centers(path), small_fit.cluster_centers_)
    tok = Tokenizer(path)
    assert tok.VOCAB_SIZE == 54
    tokens = [tok.encode(s) for s in _sketches()]
    for s, t in zip(_sketches(), tokens):
        ids = np.array([x for x in t.tolist() if 0 < x < tok.SEP]) - 1
        assert len(ids) == len(s)
        labels = _assign(np.ascontiguousarray(s[:, :2]), small_fit.cluster_centers_, dist=False)
        D = _D(s[:, :2], small_fit.cluster_centers_)
        rows = np.arange(len(s))
        assert _check_labels(D, labels) >= 0
        near_tie = (D[rows, ids] <= D.min(1) * NEAR_TIE) & (D[rows, labels] <= D.min(1) * NEAR_TIE)
        assert ((labels == ids) | near_tie).all()
    return tokens


def test_round_trip_npz(tmp_path, small_fit):
    _round_trip(str(tmp_path / "d.npz"), small_fit)


def test_round_trip_pkl_matches_npz(tmp_path, small_fit):
    pytest.importorskip("sklearn")
    a = _round_trip(str(tmp_path / "d.pkl"), small_fit)
    b = _round_trip(str(tmp_path / "d.npz"), small_fit)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ limits
def test_limits_raise_with_the_library_message():
    from sketchformer_amd import ops, _lib
    p = torch.zeros(16, 2, device="cuda")
    c = torch.zeros(4, 2, device="cuda")
    with pytest.raises(_lib.SkfError, match="only d == 2"):
        ops.kmeans_assign(torch.zeros(16, 3, device="cuda"), torch.zeros(4, 3, device="cuda"))
    with pytest.raises(_lib.SkfError, match=r"K must be in \[1, 4096\]"):
        ops.kmeans_assign(p, torch.zeros(0, 2, device="cuda"))
    with pytest.raises(_lib.SkfError, match=r"K must be in \[1, 4096\]"):
        ops.kmeans_assign(p, torch.zeros(4097, 2, device="cuda"))
    wide = torch.zeros(16, 4, device="cuda")
    with pytest.raises(_lib.SkfError, match="8-byte aligned"):
        ops.kmeans_assign(wide[:, 1:3], c)                               # base pointer 4 bytes off
    with pytest.raises(_lib.SkfError, match="8-byte aligned"):
        ops.kmeans_assign(torch.zeros(16, 3, device="cuda")[:, :2], c)   # odd row pitch
    state = ops.new_kmeans_state(p.device)
    with pytest.raises(_lib.SkfError, match=r"K must be in \[1, 4096\]"):
        ops.kmeans_step(p, torch.zeros(4097, 2, device="cuda"), state, 0)
    with pytest.raises(_lib.SkfError, match="only d == 2"):
        ops.kmeans_step(torch.zeros(16, 3, device="cuda"), torch.zeros(4, 3, device="cuda"), state, 0)
    assert _lib.load().skf_kmeans_workspace_bytes(16, 0) == 0 and _lib.load().skf_kmeans_workspace_bytes(2 ** 31, 4) == 0
    with pytest.raises(_lib.SkfError):
        ops.kmeans_assign(p.cpu(), c.cpu())                              # no CPU path
