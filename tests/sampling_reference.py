"""The selection rule of the sampled decode (include/skf.h) as written, in numpy float64, plus the acceptance and ambiguity
tests the GPU tests hold the kernels to.  params = (temperature, top_k, top_p)."""
import numpy as np

TOL = 1e-4          # the bar tests/test_gpu_decode_attention.py holds the decoder's softmax rows to


def _z(logits64, temperature):
    return np.asarray(logits64, dtype=np.float64) / float(temperature)


def _kth(z, k):
    """the k-th largest value"""
    return np.sort(z)[len(z) - k]


def _mass_above(z, e):
    """per entry: the mass of the entries with a strictly larger z (ties share one value)"""
    uz, inv = np.unique(z, return_inverse=True)               # ascending
    mass = np.bincount(inv, weights=e, minlength=len(uz))
    above = mass.sum() - np.cumsum(mass)                      # mass of strictly larger unique values
    above[-1] = 0.0
    return above[inv]


def survivors(logits64, params):
    """-> (keep (V,) bool, e (V,) float64 with the dropped entries at 0)"""
    temperature, top_k, top_p = params
    z = _z(logits64, temperature)
    V = len(z)
    with np.errstate(invalid="ignore"):
        e = np.exp(z - z.max())
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        keep = z >= _kth(z, top_k)
    e = np.where(keep, e, 0.0)
    if top_p < 1.0:
        S = e.sum()
        keep = keep & (_mass_above(z, e) < top_p * S)
        keep[z == z.max()] = True                             # (the maximum is always kept: nothing lies above it)
        e = np.where(keep, e, 0.0)
    return keep, e


def sample(logits64, params, u):
    """the token the rule draws for u"""
    keep, e = survivors(logits64, params)
    c = np.cumsum(e)
    r = u * c[-1]
    hit = np.nonzero(keep & (c > r))[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(keep)[0][-1])


def accepts(logits64, params, u, token, tol=TOL):
    """token is a survivor and u lies in its interval of the normalised survivor CDF, give or take tol"""
    keep, e = survivors(logits64, params)
    token = int(token)
    if token < 0 or token >= len(keep) or not keep[token]:
        return False
    cdf = np.cumsum(e) / e.sum()
    lo = cdf[token - 1] if token > 0 else 0.0
    return bool(lo - tol <= u <= cdf[token] + tol)


def ambiguous(logits64, params, tol=TOL):
    """the survivor set changes under a perturbation of tol: the (k+1)-th largest z lies within tol of the k-th without being
    equal to it (equal values share one fate by the rule), or some entry's mass-above lies within tol * S of top_p * S (the
    maximum, with nothing above it, is kept whatever happens)"""
    temperature, top_k, top_p = params
    z = _z(logits64, temperature)
    V = len(z)
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        zs = np.sort(z)[::-1]
        a, b = zs[top_k - 1], zs[top_k]
        if a != b and np.isfinite(a) and np.isfinite(b) and a - b <= tol:
            return True
        keep = z >= a
    if top_p < 1.0:
        with np.errstate(invalid="ignore"):
            e = np.where(keep, np.exp(z - z.max()), 0.0)
        S = e.sum()
        above = _mass_above(z, e)
        near = keep & (above > 0.0) & (np.abs(above - top_p * S) <= tol * S)
        if near.any():
            return True
    return False
