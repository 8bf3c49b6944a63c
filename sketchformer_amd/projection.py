"""2-D maps of the embedding as a product of this repository: exact t-SNE on the device (ops.tsne_affinities / ops.tsne_step /
ops.tsne_kl over skf_tsne.hip) and PCA on the host.  They serve the `tsne`, `tsne-predicted` and `pca` metrics
(metrics/visualisation.py) and the embedding-projection experiment; nothing here needs scikit-learn.

`tsne` is the exact O(N^2) algorithm of van der Maaten & Hinton (2008) with the schedule of scikit-learn's TSNE(method='exact'):
early exaggeration with momentum 0.5, then momentum 0.8, per-coordinate gains, no recentring and no early stop (every fit runs
its n_iter iterations, so a fit never reads anything back before its end).  DESIGN.md section 3k.
"""
import contextlib

import numpy as np

MAX_POINTS = 8192                # skf_tsne_*: Y fits in 64 KB of LDS, P in 256 MB
MAX_FEATURES = 1024
INIT_STD = 1e-4


def pca(x, n_components=2):
    """Principal-component scores of x (N, d) -> (N, n_components) float64: centre, numpy SVD, U * S.  The sign of a component is
    scikit-learn's svd_flip rule: the entry of largest magnitude of its left singular vector is positive."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be (N, d)")
    if not 1 <= n_components <= min(x.shape):
        raise ValueError("n_components must be in [1, min(N, d)] (got %r for x %r)" % (n_components, x.shape))
    xc = x - x.mean(axis=0)
    u, s, _ = np.linalg.svd(xc, full_matrices=False)
    top = np.argmax(np.abs(u), axis=0)
    signs = np.sign(u[top, np.arange(u.shape[1])])
    signs[signs == 0] = 1.0
    return ((u * signs) * s)[:, :n_components]


def auto_learning_rate(n_points, early_exaggeration):
    return max(n_points / float(early_exaggeration) / 4.0, 50.0)


def initial_embedding(x, init, seed):
    """The (N, 2) float32 start of a fit.  'random': RandomState(seed).standard_normal((N, 2)) * 1e-4; 'pca': the PCA scores scaled
    so that the first column's standard deviation is 1e-4; or an (N, 2) array, taken as it is."""
    N = x.shape[0]
    if isinstance(init, str):
        if init == 'random':
            return (np.random.RandomState(seed).standard_normal((N, 2)) * INIT_STD).astype(np.float32)
        if init == 'pca':
            y = pca(x, 2)
            sd = float(np.std(y[:, 0]))
            return (y / sd * INIT_STD if sd > 0.0 else y).astype(np.float32)
        raise ValueError("init must be 'random', 'pca' or an (N, 2) array (got %r)" % (init,))
    y = np.asarray(init, dtype=np.float32)
    if y.shape != (N, 2):
        raise ValueError("an init array must have shape (N, 2) = (%d, 2), got %r" % (N, y.shape))
    if not np.isfinite(y).all():
        raise ValueError("init must be finite")
    return np.array(y, dtype=np.float32)


def tsne(x, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250, learning_rate='auto', init='random',
         seed=14, device=None, return_kl=False):
    """Exact t-SNE of x (N, d), numpy in -> (N, 2) float32 numpy out (and the final KL divergence with return_kl).

    3 <= N <= 8192, d <= 1024 (columns are zero-padded to a multiple of 4, which changes no distance), 1 <= perplexity <= N - 1.
    The first exaggeration_iters iterations multiply P by early_exaggeration and use momentum 0.5, the rest use 1 and 0.8;
    learning_rate 'auto' = max(N / early_exaggeration / 4, 50).  init: see initial_embedding.  All n_iter iterations are enqueued
    on a stream of the chosen device (default: the calling thread's current device) and the result is read once, after this
    function has synchronised that stream - it is safe to call from a worker thread.  Two calls with the same arguments return
    bit-equal results."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be (N, d)")
    N, d = x.shape
    if not 3 <= N <= MAX_POINTS:
        raise ValueError("t-SNE needs 3 <= N <= %d points (got %d)" % (MAX_POINTS, N))
    if not 1 <= d <= MAX_FEATURES:
        raise ValueError("t-SNE needs 1 <= d <= %d features (got %d)" % (MAX_FEATURES, d))
    if not 1.0 <= float(perplexity) <= N - 1:
        raise ValueError("perplexity must be in [1, N - 1] = [1, %d] (got %r)" % (N - 1, perplexity))
    if not np.isfinite(x).all():
        raise ValueError("x must be finite")
    n_iter, exaggeration_iters = int(n_iter), int(exaggeration_iters)
    if n_iter < 0 or exaggeration_iters < 0:
        raise ValueError("n_iter and exaggeration_iters must not be negative")
    y0 = initial_embedding(x, init, seed)
    lr = auto_learning_rate(N, early_exaggeration) if isinstance(learning_rate, str) else float(learning_rate)
    if isinstance(learning_rate, str) and learning_rate != 'auto':
        raise ValueError("learning_rate must be 'auto' or a number (got %r)" % (learning_rate,))
    if d % 4:
        x = np.concatenate((x, np.zeros((N, 4 - d % 4), dtype=np.float32)), axis=1)

    import torch
    from . import ops
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type == 'cuda':
        dev_scope = torch.cuda.device(dev)
    else:
        dev_scope = contextlib.nullcontext()                     # the real ops refuse host tensors: there is no CPU path
    with dev_scope:
        stream = torch.cuda.Stream(device=dev) if dev.type == 'cuda' else None
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            xt = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            Y = torch.from_numpy(y0).to(dev)
            U = torch.zeros_like(Y)
            gains = torch.ones_like(Y)
            P = ops.tsne_affinities(xt, float(perplexity))
            for it in range(n_iter):
                early = it < exaggeration_iters
                ops.tsne_step(P, Y, U, gains, float(early_exaggeration) if early else 1.0, 0.5 if early else 0.8, lr)
            kl = ops.tsne_kl(P, Y) if return_kl else None
            if stream is not None:
                stream.synchronize()
            y = Y.cpu().numpy()
            kl = float(kl.cpu()[0]) if return_kl else None
    return (y, kl) if return_kl else y
