"""Exact t-SNE on the device (skf_tsne_affinities_f32 / skf_tsne_step_f32 / skf_tsne_kl_f32 through ops.tsne_* and
projection.tsne) against the float64 oracle of tests/tsne_reference.py, the projection metrics without scikit-learn, and the
embedding-projection experiment.  Every bound below is derived from the arithmetic (docstrings), none from what the kernels gave;
each test prints its figures (the device's error and the bound) before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

import tsne_reference as ref

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
AFFINITY_CASES = [(257, 32, 30.0), (65, 4, 5.0), (3, 4, 1.0), (96, 8, 95.0)]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _case_x(N, d):
    return ref.blobs(N, d, 3, 100 + N, 2.0)[0]


_AFF = {}


def _affinity_case(case):
    """(x, P_dev float32 numpy, beta_dev, P_64, beta_64) of one case, computed once."""
    if case not in _AFF:
        from sketchformer_amd import ops
        N, d, perplexity = case
        x = _case_x(N, d)
        P, beta = ops.tsne_affinities(_dev(x), perplexity, return_beta=True)
        with np.errstate(all='ignore'):
            P64, beta64 = ref.affinities(ref.distances(x), perplexity)
        _AFF[case] = (x, P.cpu().numpy(), beta.cpu().numpy(), P64, beta64)
    return _AFF[case]


def _affinity_bound(d):
    """A sequential fp32 sum of d non-negative terms is within (d + 2) u of the exact distance; the exponent beta e <= ln 1e12 ~ 28
    multiplies that relative error into p; the normaliser and the shift of the root add the same order again: 3 * 28 -> 96."""
    return 96.0 * (d + 2) * U24


@pytest.mark.parametrize("case", AFFINITY_CASES, ids=lambda c: "N%d-d%d-perp%g" % c)
def test_affinities_vs_oracle(case):
    from sketchformer_amd import ops
    N, d, perplexity = case
    x, P, beta, P64, beta64 = _affinity_case(case)
    assert P.dtype == np.float32 and P.shape == (N, N) and np.isfinite(P).all()
    assert np.array_equal(P.view(np.uint32), P.T.view(np.uint32)), "P is not symmetric bit for bit"
    assert not np.diag(P).any()
    total = P.astype(np.float64).sum()
    big = P64 >= 1e-12 * P64.max()
    rel = np.abs(P[big] - P64[big]) / P64[big]
    small = np.abs(P[~big]).max() if (~big).any() else 0.0
    bound = _affinity_bound(d)
    print("TSNE_ERR affinities N=%d d=%d perp=%g: max rel err %.3e bound %.3e ratio %.3f | |sum-1| %.2e | small entries max %.2e of %.2e"
          % (N, d, perplexity, rel.max(), bound, rel.max() / bound, abs(total - 1.0), small, 2e-12 * P64.max()))
    assert abs(total - 1.0) <= 1e-5
    assert rel.max() <= bound
    assert small <= 2e-12 * P64.max()
    # the same call through views with a larger row pitch: x inside (N, d + 4), P inside a buffer 4 columns wider than the pitch the
    # alignment rule gives N (N + 4 itself is not a multiple of 4 for an odd N)
    xw = torch.full((N, d + 4), 7.0, device="cuda")
    xw[:, :d] = _dev(x)
    pitch = (N + 3) // 4 * 4 + 4
    pw = torch.full((N, pitch), 7.0, device="cuda")
    P2, beta2 = ops.tsne_affinities(xw[:, :d], perplexity, return_beta=True, out=pw[:, :N])
    assert P2.data_ptr() == pw.data_ptr() and P2.stride(0) == pitch
    assert np.array_equal(P2.cpu().numpy().view(np.uint32), P.view(np.uint32))
    assert np.array_equal(beta2.cpu().numpy().view(np.uint64), beta.view(np.uint64))
    assert bool((pw[:, N:] == 7.0).all()), "columns past N were written"


@pytest.mark.parametrize("case", AFFINITY_CASES, ids=lambda c: "N%d-d%d-perp%g" % c)
def test_affinities_beta_vs_oracle(case):
    """beta relative error <= the affinity bound / 28.

    The two extreme perplexities have roots of their own kind.  At perplexity 1 the root is where exp(-beta e) underflows to zero
    (beta e = 745.13), on the device as in numpy.  At perplexity N - 1 the entropy target is the maximum, reached only as
    beta -> 0: H - log(N - 1) is negative at every beta, and both the kernel and the oracle take its sign from the form without
    cancellation (include/skf.h), so every row halves 64 times and ends at 2^-63 on both sides.  (Taken from log S + beta sum e p / S,
    that sign is rounding noise below beta ~ 1e-9: the first version of this code and of the oracle disagreed there by a factor 1e9,
    and the oracle's own betas spread from 1e-19 to 1e-10 over the rows.)"""
    N, d, perplexity = case
    x, P, beta, P64, beta64 = _affinity_case(case)
    rel = np.abs(beta - beta64) / beta64
    bound = _affinity_bound(d) / 28.0
    print("TSNE_ERR beta N=%d d=%d perp=%g: max rel err %.3e bound %.3e ratio %.3f" % (N, d, perplexity, rel.max(), bound, rel.max() / bound))
    assert np.isfinite(beta).all() and (beta > 0).all()
    assert rel.max() <= bound


def test_degenerate_rows():
    from sketchformer_amd import ops
    N, d = 90, 8
    x = _case_x(N, d)
    x[1] = x[0]
    x[60:] = x[60]                                                               # a third of the points are one point
    P, beta = ops.tsne_affinities(_dev(x), 12.0, return_beta=True)
    P, beta = P.cpu().numpy(), beta.cpu().numpy()
    assert np.isfinite(P).all() and np.isfinite(beta).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 1e-5
    assert np.array_equal(P.view(np.uint32), P.T.view(np.uint32)) and not np.diag(P).any()
    for group in ([0, 1], list(range(60, N))):
        others = np.setdiff1d(np.arange(N), group)
        first = P[group[0], others].view(np.uint32)
        for r in group[1:]:
            assert np.array_equal(P[r, others].view(np.uint32), first), "identical rows %d and %d differ" % (group[0], r)
        assert len(np.unique(beta[group].view(np.uint64))) == 1
        inner = P[np.ix_(group, group)][~np.eye(len(group), dtype=bool)]
        assert len(np.unique(inner.view(np.uint32))) == 1                        # the mutual entries are one value too
    with np.errstate(all='ignore'):
        P64, _ = ref.affinities(ref.distances(x), 12.0)
    big = P64 >= 1e-12 * P64.max()
    assert (np.abs(P[big] - P64[big]) / P64[big]).max() <= _affinity_bound(d)


_STATE = {}


def _state(N):
    """Per N: the device's P (tensor and float64 numpy), the random 1e-4 init, and the oracle's float64 state after 60 iterations
    on that P, cast to float32."""
    if N not in _STATE:
        from sketchformer_amd import ops
        d, perplexity = (32, 30.0) if N == 257 else (4, 5.0)
        P = ops.tsne_affinities(_dev(_case_x(N, d)), perplexity)
        P64 = P.cpu().numpy().astype(np.float64)
        Y0 = ref.random_init(N, 14)
        Y60 = ref.descend(P64, Y0, 60).astype(np.float32)
        _STATE[N] = (P, P64, Y0, Y60)
    return _STATE[N]


@pytest.mark.parametrize("N", [257, 65])
@pytest.mark.parametrize("state", ["init-ex12", "iter60-ex1"])
def test_one_step_gradient(N, state):
    """|g_dev - g_64| <= (N + 16) u A_i per component, A_i = 4 sum_j (ex P_ij + q_ij / Z) q_ij |y_i - y_j| from the oracle: the
    worst case of a length-N fp32 sum in any order ((N - 1) u A), plus 16 u for the roundings inside a term and of Z."""
    from sketchformer_amd import ops
    P, P64, Y0, Y60 = _state(N)
    Y, ex = (Y0, 12.0) if state == "init-ex12" else (Y60, 1.0)
    g64, A = ref.gradient(P64, Y, ex)
    Yd = _dev(Y)
    g = ops.tsne_step(P, Yd, torch.zeros_like(Yd), torch.ones_like(Yd), ex, 0.5, 50.0, return_grad=True).cpu().numpy()
    err, bound = np.abs(g - g64), (N + 16) * U24 * A
    ratio = (err / bound).max()
    print("TSNE_ERR gradient N=%d %s: max |g| %.3e, worst err/bound %.4f" % (N, state, np.abs(g64).max(), ratio))
    assert np.isfinite(g).all() and (err <= bound).all()


@pytest.mark.parametrize("momentum", [0.5, 0.8])
def test_update_rule_is_exact(momentum):
    """Given the device's own gradient, Y', U' and gains' are update_f32 bit for bit: one float32 rounding per operation."""
    from sketchformer_amd import ops
    N = 257
    P, P64, Y0, Y60 = _state(N)
    rng = np.random.RandomState(5)
    U = (rng.standard_normal((N, 2)) * 0.05).astype(np.float32)
    U[:40] = 0.0                                                                 # U = 0: U g < 0 is false -> gain * 0.8
    gains = (0.5 + rng.random_sample((N, 2)) * 2.0).astype(np.float32)
    gains[30:90] = np.float32(0.0101)                                            # * 0.8 falls under the floor of 0.01
    lr = 53.5
    Yd, Ud, gd = _dev(Y60), _dev(U), _dev(gains)
    g = ops.tsne_step(P, Yd, Ud, gd, 1.0, momentum, lr, return_grad=True).cpu().numpy()
    Y2, U2, gains2 = ref.update_f32(Y60, U, gains, g, momentum, lr)
    inc = (U * g) < 0
    assert inc.any() and (~inc).any() and (gains2 == np.float32(0.01)).any() and not inc[:40].any()
    for name, got, want in (("gains", gd, gains2), ("U", Ud, U2), ("Y", Yd, Y2)):
        got = got.cpu().numpy()
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, "%s: %d of %d elements differ from the float32 rule" % (name, bad, got.size)


@pytest.mark.parametrize("N", [257, 65])
def test_kl_vs_oracle(N):
    """Only q and its row sums are fp32: q within a few u, z_i and Z within (N / 64 + 8) u, so log(P Z / q) moves by that much in
    absolute terms and KL, whose P-weights sum to 1, by at most (N + 16) u relative to a KL of order 1 or more."""
    from sketchformer_amd import ops
    P, P64, Y0, Y60 = _state(N)
    for name, Y in (("iter60", Y60), ("init", Y0)):
        want = ref.kl(P64, Y)
        got = float(ops.tsne_kl(P, _dev(Y)).cpu()[0])
        rel, bound = abs(got - want) / abs(want), (N + 16) * U24
        print("TSNE_ERR kl N=%d %s: KL %.6f rel err %.3e bound %.3e ratio %.4f" % (N, name, want, rel, bound, rel / bound))
        assert rel <= bound


def test_short_trajectory_across_the_schedule_switch():
    """10 iterations, the switch after 5: max|Y_dev - Y_64| / max|Y_64| <= 32 e32, e32 the same figure for the numpy float32
    restatement of the loop.  The iteration amplifies differences (the restatement's error grows 14-fold from 1 to 10 iterations)
    and the device's summation order is neither numpy's nor the oracle's: hence a factor, and no longer trajectories."""
    from sketchformer_amd import projection
    N = 257
    x = _case_x(N, 32)
    Y0 = ref.random_init(N, 14)
    P64, _ = ref.affinities(ref.distances(x), 30.0)
    Y64 = ref.descend(P64, Y0, 10, exaggeration_iters=5)
    Y32 = ref.descend_f32(P64, Y0, 10, exaggeration_iters=5)
    Yd = projection.tsne(x, perplexity=30.0, n_iter=10, exaggeration_iters=5, init=Y0)
    scale = np.abs(Y64).max()
    e32 = np.abs(Y32 - Y64).max() / scale
    edev = np.abs(Yd - Y64).max() / scale
    print("TSNE_ERR trajectory N=%d 10 iterations: device %.3e, float32 restatement e32 %.3e, ratio %.3f (bar 32)" % (N, edev, e32, edev / e32))
    assert np.isfinite(Yd).all() and edev <= 32.0 * e32


def test_whole_fit_separates_the_blobs():
    """A sanity bound (the gradient, update and KL tests carry correctness): the device's final KL lies inside the oracle's own
    seed-to-seed range over init seeds 0..3, widened by the 10 % that range itself spans."""
    from sketchformer_amd import projection
    x, labels = ref.blobs(96, 8, 3, 3, 4.0)
    Y, kl = projection.tsne(x, perplexity=10.0, n_iter=1000, seed=14, return_kl=True)
    P64, _ = ref.affinities(ref.distances(x), 10.0)
    kls = [ref.kl(P64, ref.descend(P64, ref.random_init(96, s), 1000)) for s in range(4)]
    print("TSNE_ERR whole fit: device KL %.4f, oracle seeds 0..3 %s, 1-NN accuracy %.3f" % (kl, ["%.4f" % k for k in kls], ref.one_nn_accuracy(Y, labels)))
    assert Y.shape == (96, 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and np.isfinite(kl)
    assert ref.one_nn_accuracy(Y, labels) == 1.0
    assert 0.90 * min(kls) <= kl <= 1.10 * max(kls)


def test_fit_is_deterministic():
    from sketchformer_amd import projection
    x = _case_x(257, 32)
    a, ka = projection.tsne(x, n_iter=100, return_kl=True)
    b, kb = projection.tsne(x, n_iter=100, return_kl=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.float64(ka).tobytes() == np.float64(kb).tobytes()
    assert np.isfinite(a).all() and len(np.unique(a, axis=0)) == 257
    c = projection.tsne(x, n_iter=100, init='pca')                               # the other built-in start runs too
    assert np.isfinite(c).all() and not np.array_equal(a, c)


def test_limits_are_refused_before_any_launch():
    from sketchformer_amd import ops
    from sketchformer_amd._lib import SkfError

    def refused(x, perplexity, N_out=None, match=None):
        N = x.shape[0] if N_out is None else N_out
        out = torch.full((N, (N + 3) // 4 * 4), 7.0, device="cuda")[:, :N] if N <= 256 else None
        with pytest.raises(SkfError, match=match):
            ops.tsne_affinities(x, perplexity, out=out)
        torch.cuda.synchronize()
        assert out is None or bool((out == 7.0).all()), "a refused call wrote to P"

    refused(torch.zeros(2, 4, device="cuda"), 1.0, match=r"N must be in \[3, 8192\]")
    refused(torch.zeros(8193, 4, device="cuda"), 30.0, match=r"N must be in \[3, 8192\]")
    refused(torch.randn(16, 6, device="cuda"), 5.0, match="multiple of 4")
    refused(torch.randn(16, 8, device="cuda"), 16.0, match="perplexity")
    refused(torch.randn(16, 8, device="cuda"), 0.5, match="perplexity")
    refused(torch.randn(16, 12, device="cuda")[:, 1:9], 5.0, match="16-byte aligned")       # base pointer off by 4 bytes
    refused(torch.randn(16, 10, device="cuda")[:, :8], 5.0, match="16-byte aligned")        # row pitch 40 bytes
    # the step and the KL refuse a P whose rows are not 16-byte aligned, and (N, 2) arrays that are not contiguous
    P = torch.zeros(18, 18, device="cuda")
    Y = torch.zeros(18, 2, device="cuda")
    with pytest.raises(SkfError, match="16-byte aligned"):
        ops.tsne_step(P, Y, Y.clone(), Y.clone(), 1.0, 0.5, 50.0)
    with pytest.raises(SkfError, match="16-byte aligned"):
        ops.tsne_kl(P, Y)
    with pytest.raises(ValueError):
        ops.tsne_step(torch.zeros(16, 16, device="cuda"), torch.zeros(16, 4, device="cuda")[:, :2], Y[:16].clone(), Y[:16].clone(), 1.0, 0.5, 50.0)
    with pytest.raises(SkfError, match="no CPU fallback"):
        ops.tsne_affinities(torch.zeros(16, 8), 5.0)


# ------------------------------------------------------------------ the plugin surface (set up as tests/test_gpu_plugin.py does)
SMALL = "num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"
DATA = "max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"


def _build(tmp_path, exp_id="t0", base="batch_size=8,num_epochs=1,log_every=4", specific=SMALL):
    from sketchformer_amd import models, dataloaders
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams(DATA), None)
    model = Model(Model.parse_hparams(base=base, specific=specific), dataset, str(tmp_path), exp_id)
    return model, dataset


def test_projection_metrics_and_experiment_without_scikit_learn(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, 'sklearn', None)                            # `import sklearn` raises ImportError
    from sketchformer_amd import experiments, metrics
    model, dataset = _build(tmp_path, "pj")
    n_valid = len(dataset.get_all_data_from("valid")[0])
    chosen = {m: metrics.build_metric_by_name(m, model.hps) for m in ("tsne", "tsne-predicted", "pca")}
    model.compute_metrics_from(chosen)
    for m in ("tsne", "tsne-predicted", "pca"):
        proj = chosen[m].get_data_for_plot()
        assert proj.ndim == 2 and proj.shape[1] == 3 and np.isfinite(proj).all() and len(proj) > 10, (m, proj)
        assert len(np.unique(proj[:, :2], axis=0)) > 1, m
    Exp = experiments.get_experiment_by_name("embedding-projection")
    exp = Exp(Exp.parse_hparams("n_samples=64,n_iter=50"), "p0", str(tmp_path))
    target = exp.compute(model)
    out = np.load(target, allow_pickle=True)
    n = min(64, n_valid)
    assert out["projection"].shape == (n, 2) and np.isfinite(out["projection"]).all() and np.isfinite(out["kl_divergence"])
    assert out["y"].shape == (n,) and out["pred_y"].shape == (n,) and np.array_equal(out["rows"], np.arange(n_valid)[:n])
    assert len(np.unique(out["projection"], axis=0)) > 1
    png = os.path.splitext(target)[0] + ".png"
    assert os.path.exists(png) and os.path.getsize(png) > 1000
    exp = Exp(Exp.parse_hparams("n_samples=20,method=pca,target_file=pca.npz"), "p1", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    assert out["projection"].shape == (20, 2) and np.isnan(out["kl_divergence"]) and len(out["rows"]) == 20
    assert sys.modules['sklearn'] is None
