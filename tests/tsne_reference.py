"""float64 numpy oracle of exact t-SNE (van der Maaten & Hinton 2008, scikit-learn's method='exact' without its tolerance exit and
without its early stop) for tests/test_gpu_tsne.py and tests/test_projection_cpu.py.  Written from the definitions in include/skf.h;
it shares no code with sketchformer_amd."""
import numpy as np

STEPS = 64


def blobs(N, d, C, seed, sep):
    """Gaussian blobs: centres standard_normal * sep, unit noise, labels arange(N) % C -> (x float32 (N, d), labels)."""
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((C, d)) * sep
    labels = np.arange(N) % C
    return (centres[labels] + rng.standard_normal((N, d))).astype(np.float32), labels


def distances(x):
    """Squared Euclidean distances of the float32 rows of x, in float64 (direct differences)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    D = np.zeros((len(x), len(x)))
    for k in range(x.shape[1]):
        df = x[:, None, k] - x[None, :, k]
        D += df * df
    return D


def row_entropies(D, beta):
    """(H, S, p) of every row at its beta: p_j = exp(-beta e_j) over j != i, e_j = D_ij - min_{j != i} D_ij."""
    N = len(D)
    off = ~np.eye(N, dtype=bool)
    e = D - np.where(off, D, np.inf).min(axis=1, keepdims=True)
    e[~off] = 0.0
    p = np.where(off, np.exp(-beta[:, None] * e), 0.0)
    S = p.sum(axis=1)
    H = np.log(S) + beta * (e * p).sum(axis=1) / S
    return H, S, p


KL_FORM_ABOVE = 0.75


def _f(eps):
    """(1 + eps) log(1 + eps) - eps >= 0, by its series eps^2/2 - eps^3/6 + eps^4/12 - eps^5/20 + eps^6/30 below |eps| = 1e-3;
    1 at eps <= -1 (the limit)."""
    with np.errstate(all='ignore'):
        direct = np.where(1.0 + eps > 0.0, (1.0 + eps) * np.log1p(np.maximum(eps, -1.0)) - eps, -eps)
    series = eps * eps * (0.5 + eps * (-1.0 / 6.0 + eps * (1.0 / 12.0 + eps * (-1.0 / 20.0 + eps * (1.0 / 30.0)))))
    return np.where(np.abs(eps) < 1e-3, series, direct)


def entropy_differences(D, beta, perplexity):
    """(H - log(perplexity), S, p) of every row at its beta, the quantity whose sign steers the bisection.  Two forms of the same
    number, n = N - 1 being the number of neighbours:
      far from uniform (S / n <= 0.75):  log S + beta sum e_j p_j / S - log(perplexity), the definition as it stands;
      near uniform (S / n > 0.75):       log(n / perplexity) - (1 / n) sum_j f(n w_j - 1), w_j = p_j / S,
    because H - log n = -KL(w || uniform) = -(1 / n) sum_j f(n w_j - 1) with f(x) = (1 + x) log(1 + x) - x >= 0 (sum_j (n w_j - 1)
    is zero), and n w_j - 1 = (expm1(-beta e_j) - m) / (1 + m), m = mean_j expm1(-beta e_j).  In the first form log S and
    beta sum e p / S cancel as the row approaches uniformity, and at perplexity close to n the sign of the difference is then
    rounding noise; in the second every term is non-negative and keeps its relative accuracy down to beta = 2^-63."""
    N = len(D)
    n = N - 1
    off = ~np.eye(N, dtype=bool)
    H, S, p = row_entropies(D, beta)
    naive = H - np.log(perplexity)
    e = D - np.where(off, D, np.inf).min(axis=1, keepdims=True)
    e[~off] = 0.0
    em = np.where(off, np.expm1(-beta[:, None] * e), 0.0)
    m = em.sum(axis=1) / n
    with np.errstate(all='ignore'):
        eps = (em - m[:, None]) / (1.0 + m[:, None])
    kl_form = np.log(n / perplexity) - np.where(off, _f(eps), 0.0).sum(axis=1) / n
    return np.where(S / n > KL_FORM_ABOVE, kl_form, naive), S, p


def affinities(D, perplexity, steps=STEPS):
    """-> (P joint (N, N), beta (N,)): per row `steps` bisection steps on beta from 1 with bounds (0, inf), scikit-learn's rule,
    no early exit, steered by entropy_differences; beta and the conditionals are those of the last evaluation;
    P = (cond + cond.T) / 2N."""
    D = np.asarray(D, dtype=np.float64)
    N = len(D)
    beta, lo, hi = np.ones(N), np.zeros(N), np.full(N, np.inf)
    for _ in range(steps):
        diff, S, p = entropy_differences(D, beta, perplexity)
        used = beta.copy()
        up = diff > 0.0
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        with np.errstate(invalid='ignore', over='ignore'):
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) * 0.5), (beta + lo) * 0.5)
    cond = p / S[:, None]
    return (cond + cond.T) / (2.0 * N), used


def _pairs(Y):
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    qz = q.copy()
    np.fill_diagonal(qz, 0.0)
    return diff, q, qz.sum()


def gradient(P, Y, exaggeration):
    """-> (g (N, 2), A (N, 2)): the gradient 4 sum_j (exaggeration P_ij - q_ij / Z) q_ij (y_i - y_j) and, per component, the sum of
    the absolute values of its terms A_i = 4 sum_j (exaggeration P_ij + q_ij / Z) q_ij |y_i - y_j|."""
    P = np.asarray(P, dtype=np.float64)
    diff, q, Z = _pairs(Y)
    g = 4.0 * (((exaggeration * P - q / Z) * q)[:, :, None] * diff).sum(axis=1)
    A = 4.0 * (((exaggeration * P + q / Z) * q)[:, :, None] * np.abs(diff)).sum(axis=1)
    return g, A


def update(Y, U, gains, g, momentum, lr):
    """scikit-learn's gains / momentum update in the dtype of its arguments -> (Y', U', gains')."""
    gains = np.where(U * g < 0.0, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    U = momentum * U - lr * (gains * g)
    return Y + U, U, gains


def update_f32(Y, U, gains, g, momentum, lr):
    """The same rule in numpy float32, one rounding per operation -> (Y', U', gains') float32."""
    f = np.float32
    Y, U, gains, g = (np.asarray(a, dtype=f) for a in (Y, U, gains, g))
    inc = (U * g) < f(0.0)
    gn = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
    gn = np.maximum(gn, f(0.01))
    t1 = f(momentum) * U
    t2 = gn * g
    t3 = f(lr) * t2
    U2 = (t1 - t3).astype(f)
    return (Y + U2).astype(f), U2, gn


def step(P, Y, U, gains, exaggeration, momentum, lr):
    """One iteration in float64 -> (g, abs_bound_terms, Y', U', gains')."""
    g, A = gradient(P, Y, exaggeration)
    Y2, U2, gains2 = update(np.asarray(Y, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(gains, dtype=np.float64),
                            g, momentum, lr)
    return g, A, Y2, U2, gains2


def kl(P, Y):
    """sum over P_ij > 0 of P_ij log(P_ij / Q_ij), Q = q / Z."""
    P = np.asarray(P, dtype=np.float64)
    _, q, Z = _pairs(Y)
    m = P > 0.0
    return float((P[m] * np.log(P[m] / (q[m] / Z))).sum())


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def random_init(N, seed):
    return (np.random.RandomState(seed).standard_normal((N, 2)) * 1e-4).astype(np.float32)


def descend(P, Y0, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250, lr=None):
    """The schedule in float64 from Y0: exaggeration and momentum 0.5 for the first exaggeration_iters iterations, then 1 and 0.8."""
    N = len(P)
    lr = auto_learning_rate(N, early_exaggeration) if lr is None else lr
    Y = np.asarray(Y0, dtype=np.float64).copy()
    U, gains = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iter):
        early = it < exaggeration_iters
        _, _, Y, U, gains = step(P, Y, U, gains, early_exaggeration if early else 1.0, 0.5 if early else 0.8, lr)
    return Y


def descend_f32(P, Y0, n_iter, early_exaggeration=12.0, exaggeration_iters=250, lr=None):
    """The same loop restated in numpy float32 throughout (pairs, sums, Z, gradient, update_f32): the error a float32
    implementation with numpy's summation order makes."""
    f = np.float32
    P = np.asarray(P, dtype=f)
    N = len(P)
    lr = auto_learning_rate(N, early_exaggeration) if lr is None else lr
    Y = np.asarray(Y0, dtype=f).copy()
    U, gains = np.zeros_like(Y), np.ones_like(Y)
    for it in range(n_iter):
        early = it < exaggeration_iters
        ex, mom = (f(early_exaggeration), 0.5) if early else (f(1.0), 0.8)
        diff = Y[:, None, :] - Y[None, :, :]
        q = f(1.0) / (f(1.0) + (diff * diff).sum(axis=2, dtype=f))
        qz = q.copy()
        np.fill_diagonal(qz, f(0.0))
        Z = qz.sum(dtype=f)
        g = f(4.0) * (((ex * P - q / Z) * q)[:, :, None] * diff).sum(axis=1, dtype=f)
        Y, U, gains = update_f32(Y, U, gains, g, mom, lr)
    return Y


def fit(x, perplexity, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250, seed=14, init=None):
    """-> (Y float64 (N, 2), KL): affinities of x, then the schedule from random_init(N, seed) (or the (N, 2) array `init`)."""
    P, _ = affinities(distances(x), perplexity)
    Y0 = random_init(len(P), seed) if init is None else init
    Y = descend(P, Y0, n_iter, early_exaggeration, exaggeration_iters)
    return Y, kl(P, Y)


def one_nn_accuracy(Y, labels):
    """Share of points whose nearest other point in Y carries their label."""
    D = distances(np.asarray(Y, dtype=np.float32))
    np.fill_diagonal(D, np.inf)
    return float(np.mean(np.asarray(labels)[D.argmin(axis=1)] == np.asarray(labels)))
