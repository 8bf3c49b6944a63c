"""Host side of the embedding maps: projection.pca against the eigen-decomposition, the pca metric without scikit-learn, the float64
t-SNE oracle (tests/tsne_reference.py) held to the properties that define it, and projection.tsne's argument checks and schedule."""
import sys

import numpy as np
import pytest

import tsne_reference as ref


def _pca_cases():
    return [np.random.RandomState(0).standard_normal((200, 16)) * np.linspace(3.0, 0.2, 16), ref.blobs(96, 8, 3, 3, 4.0)[0]]


@pytest.mark.parametrize("case", [0, 1])
def test_pca_is_the_eigen_decomposition(case):
    from sketchformer_amd.projection import pca
    x = np.asarray(_pca_cases()[case], dtype=np.float64)
    y = pca(x, 2)
    assert y.shape == (len(x), 2) and y.dtype == np.float64
    xc = x - x.mean(axis=0)
    w, v = np.linalg.eigh(xc.T @ xc / len(x))
    var = (y * y).sum(axis=0) / len(x)
    np.testing.assert_allclose(var, w[::-1][:2], rtol=1e-10)                     # the two largest eigenvalues, in order
    assert abs((y[:, 0] * y[:, 1]).sum()) <= 1e-10 * len(x) * np.sqrt(var[0] * var[1])      # uncorrelated columns
    assert np.abs(y.mean(axis=0)).max() <= 1e-10 * np.sqrt(var[0])
    for c in range(2):
        s = xc @ v[:, -1 - c]
        s = s if np.dot(s, y[:, c]) > 0 else -s                                  # an eigenvector's sign is free; the rule is checked below
        np.testing.assert_allclose(y[:, c], s, atol=1e-9 * np.abs(s).max())
        assert y[np.argmax(np.abs(y[:, c])), c] > 0                              # svd_flip: largest |u| entry (same row as largest |u s|)


def test_pca_sign_rule_on_a_constructed_case():
    from sketchformer_amd.projection import pca
    # centred points on two orthogonal axes; the entry of largest magnitude along each axis is NEGATIVE in these coordinates
    x = np.array([[-5.0, 0.0, 0.0], [3.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 1.5, 0.0], [0.0, 0.5, 0.0]])
    y = pca(x, 2)
    np.testing.assert_allclose(y[:, 0], [5.0, -3.0, -2.0, 0.0, 0.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(y[:, 1], [0.0, 0.0, 0.0, 2.0, -1.5, -0.5], atol=1e-12)
    np.testing.assert_allclose(pca(-x, 2), y, atol=1e-12)                        # the rule, not the input's orientation, fixes the sign


def test_pca_metric_needs_no_scikit_learn(monkeypatch):
    monkeypatch.setitem(sys.modules, 'sklearn', None)                            # `import sklearn` raises ImportError
    loaded = {m for m in sys.modules if m.startswith('sklearn.')}                # (other tests of the process may have used it)
    from sketchformer_amd.metrics import visualisation
    rng = np.random.RandomState(1)
    n = 60
    y = np.arange(n) % 4
    pred_z = rng.standard_normal((n, 16)) + y[:, None]
    data = (None, y, None, (y + 1) % 4, pred_z, None, None, None, False)
    out = visualisation.PCAProjection.compute(visualisation.PCAProjection.__new__(visualisation.PCAProjection), data)
    feats, labels = visualisation._select(y, pred_z, y)
    assert out.shape == (len(feats), 3) and len(feats) == n and np.isfinite(out).all()
    np.testing.assert_array_equal(out[:, 2], labels)
    assert len(np.unique(out[:, :2], axis=0)) > 1
    # fewer than three rows: zeros for (x, y), from the t-SNE helper as well
    small = visualisation.PCAProjection.compute(visualisation.PCAProjection.__new__(visualisation.PCAProjection),
                                                (None, y[:2], None, y[:2], pred_z[:2], None, None, None, False))
    assert small.shape == (2, 3) and not small[:, :2].any()
    assert visualisation._tsne(pred_z[:2]).shape == (2, 2) and not visualisation._tsne(pred_z[:2]).any()
    assert sys.modules['sklearn'] is None and {m for m in sys.modules if m.startswith('sklearn.')} == loaded     # nothing imported it


@pytest.fixture(scope="module")
def blob_fit():
    x, labels = ref.blobs(96, 8, 3, 3, 4.0)
    D = ref.distances(x)
    P, beta = ref.affinities(D, 10.0)
    return x, labels, D, P, beta


def test_oracle_affinities(blob_fit):
    x, labels, D, P, beta = blob_fit
    assert np.array_equal(P, P.T) and not np.diag(P).any()
    assert abs(P.sum() - 1.0) <= 1e-12
    H, _, _ = ref.row_entropies(D, beta)
    assert np.abs(H - np.log(10.0)).max() <= 1e-9
    assert np.array_equal(D, D.T) and not np.diag(D).any()


def test_oracle_entropy_difference_forms_agree_and_the_maximum_perplexity_has_one_answer(blob_fit):
    """The well-conditioned form of H - log(perplexity) is the same number as the definition wherever the definition is itself
    accurate, and at perplexity N - 1 (target = the maximum entropy, reached only as beta -> 0) every row halves 64 times."""
    x, labels, D, P, beta = blob_fit
    N = len(D)
    for b in (1e-6, 1e-5, 1e-4):                                             # rows near uniformity: the second form is in use
        bb = np.full(N, b)
        diff, S, _ = ref.entropy_differences(D, bb, 40.0)
        assert (S / (N - 1) > ref.KL_FORM_ABOVE).all()
        H, _, _ = ref.row_entropies(D, bb)
        assert np.abs(diff - (H - np.log(40.0))).max() <= 1e-13
    diff, _, _ = ref.entropy_differences(D, np.full(N, 2.0 ** -60), N - 1.0)
    assert (diff < 0.0).all()                                                # the definition gives exactly 0 or noise here
    _, b95 = ref.affinities(D, N - 1.0)
    assert (b95 == 2.0 ** -63).all()


# The oracle's final KL on these blobs over init seeds 0..7 was 0.348 - 0.396 when this was written (the issue that asked for the
# oracle quotes 0.334 - 0.372 for its own draw of the blobs): the window is both ranges with the 10 % seed-to-seed margin of the
# whole-fit GPU test.  It is a sanity window for the schedule (a fit that never leaves exaggeration, or diverges, is far outside).
KL_LO, KL_HI = 0.90 * 0.334, 1.10 * 0.396


def test_oracle_fit_separates_the_blobs(blob_fit):
    x, labels, D, P, beta = blob_fit
    Y = ref.descend(P, ref.random_init(96, 0), 1000)
    assert np.isfinite(Y).all() and ref.one_nn_accuracy(Y, labels) == 1.0
    assert KL_LO <= ref.kl(P, Y) <= KL_HI


def test_oracle_update_f32_is_the_rule_in_float32():
    rng = np.random.RandomState(2)
    Y, U, g = (rng.standard_normal((50, 2)).astype(np.float32) for _ in range(3))
    gains = np.abs(rng.standard_normal((50, 2))).astype(np.float32)
    U[:5] = 0.0
    gains[5:10] = 0.011
    Y2, U2, gains2 = ref.update_f32(Y, U, gains, g, 0.8, 200.0)
    assert Y2.dtype == U2.dtype == gains2.dtype == np.float32
    np.testing.assert_array_equal(gains2[:5], np.maximum(gains[:5] * np.float32(0.8), np.float32(0.01)))      # U = 0: not an increase
    assert (gains2 >= np.float32(0.01)).all() and (gains2[5:10][(U * g)[5:10] >= 0] == np.float32(0.01)).all()
    Y64, U64, gains64 = ref.update(*(a.astype(np.float64) for a in (Y, U, gains, g)), 0.8, 200.0)
    np.testing.assert_allclose(Y2, Y64, rtol=1e-5, atol=1e-4)


def test_tsne_argument_checks():
    from sketchformer_amd.projection import tsne
    x = np.random.RandomState(0).standard_normal((20, 8)).astype(np.float32)
    for bad in (0.5, 20, 25.0):
        with pytest.raises(ValueError, match="perplexity"):
            tsne(x, perplexity=bad)
    with pytest.raises(ValueError, match="3 <= N"):
        tsne(x[:2], perplexity=1.0)
    with pytest.raises(ValueError, match="3 <= N"):
        tsne(np.zeros((8193, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        tsne(x, perplexity=5.0, init=np.zeros((20, 3)))
    with pytest.raises(ValueError, match="shape"):
        tsne(x, perplexity=5.0, init=np.zeros((19, 2)))
    with pytest.raises(ValueError, match="init must be"):
        tsne(x, perplexity=5.0, init='spectral')
    with pytest.raises(ValueError, match="finite"):
        tsne(np.where(np.arange(8) == 3, np.nan, x), perplexity=5.0)
    with pytest.raises(ValueError, match="learning_rate"):
        tsne(x, perplexity=5.0, learning_rate='fast')


def test_initial_embedding():
    from sketchformer_amd.projection import initial_embedding
    x = ref.blobs(40, 8, 3, 3, 4.0)[0]
    y = initial_embedding(x, 'random', 14)
    assert y.dtype == np.float32 and np.array_equal(y, ref.random_init(40, 14))
    y = initial_embedding(x, 'pca', 14)
    assert y.dtype == np.float32 and y.shape == (40, 2) and np.std(y[:, 0]) == pytest.approx(1e-4, rel=1e-5)
    given = np.arange(80, dtype=np.float64).reshape(40, 2)
    y = initial_embedding(x, given, 14)
    assert y.dtype == np.float32 and np.array_equal(y, given)


def test_fit_driver_schedule(monkeypatch):
    """projection.tsne with the three device calls replaced by the float64 oracle: the recorded schedule, and the oracle's own result."""
    import torch
    from sketchformer_amd import ops, projection
    x = ref.blobs(30, 8, 3, 3, 4.0)[0]
    calls = []

    def affinities(xt, perplexity, return_beta=False):
        return torch.from_numpy(ref.affinities(ref.distances(xt.numpy()), perplexity)[0])

    def step(P, Y, U, gains, exaggeration, momentum, learning_rate, return_grad=False):
        calls.append((exaggeration, momentum, learning_rate))
        _, _, Y2, U2, g2 = ref.step(P.numpy(), Y.numpy(), U.numpy(), gains.numpy(), exaggeration, momentum, learning_rate)
        for t, a in ((Y, Y2), (U, U2), (gains, g2)):
            t.copy_(torch.from_numpy(a))                                         # in place, as the device call

    def kl(P, Y):
        return torch.tensor([ref.kl(P.numpy(), Y.numpy())], dtype=torch.float64)

    monkeypatch.setattr(ops, "tsne_affinities", affinities)
    monkeypatch.setattr(ops, "tsne_step", step)
    monkeypatch.setattr(ops, "tsne_kl", kl)
    y, k = projection.tsne(x, perplexity=5.0, n_iter=6, exaggeration_iters=3, device='cpu', return_kl=True)
    lr = max(30 / 12.0 / 4.0, 50.0)
    assert calls == [(12.0, 0.5, lr)] * 3 + [(1.0, 0.8, lr)] * 3
    assert y.shape == (30, 2) and y.dtype == np.float32 and np.isfinite(k)
    calls.clear()
    projection.tsne(x, perplexity=5.0, n_iter=2, exaggeration_iters=250, early_exaggeration=4.0, learning_rate=70.0, device='cpu')
    assert calls == [(4.0, 0.5, 70.0)] * 2
    calls.clear()
    big = np.zeros((4800, 4), dtype=np.float32)
    big[:, 0] = np.arange(4800)
    monkeypatch.setattr(ops, "tsne_affinities", lambda xt, perplexity, return_beta=False: torch.zeros(1, 1))
    monkeypatch.setattr(ops, "tsne_step", lambda P, Y, U, gains, ex, mom, lr, return_grad=False: calls.append(lr))
    projection.tsne(big, n_iter=1, device='cpu')
    assert calls == [100.0]                                          # above the floor of 50


def test_embedding_projection_experiment_is_registered():
    from sketchformer_amd import experiments
    Exp = experiments.get_experiment_by_name('embedding-projection')
    got = dict(Exp.specific_default_hparams().values())
    want = dict(set_type='valid', n_samples=5000, method='tsne', perplexity=30.0, n_iter=1000, init='random', target_file='projection.npz')
    assert {k: got[k] for k in want} == want
