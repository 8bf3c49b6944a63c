"""Embedding retrieval: exact k-nearest-neighbour ranking on the device (ops.knn_topk) and the scores computed from a ranking.

The reference's README names retrieval as the third use of the learned embedding (beside classification and reconstruction)
and ships no code for it; the definitions here are the usual ones: a gallery row is relevant to a query when it carries the
query's label, and

    AP_q = (1 / min(k, R_q)) * sum_{j=1..k} rel_q(j) * (hits among the first j) / j

with R_q the number of relevant gallery rows (over the WHOLE gallery, minus the query itself under leave-one-out).
Host side: numpy in, numpy out; only ``retrieve`` touches the device.
"""
import numpy as np


def retrieve(query_z, gallery_z, k, metric='l2', exclude_self=False, query_block=8192, device=None, exclude_rows=None):
    """-> (indices int32 (Q, k), distances float32 (Q, k)): the k nearest gallery rows of every query, nearest first.
    The gallery is uploaded once and the queries walk through in blocks of ``query_block`` rows, so device memory stays bounded
    for any Q.  exclude_self: query i IS gallery row i and is left out of its own ranking; exclude_rows (Q,) names the gallery
    row of each query instead (a subsample of the gallery as queries; -1 = none)."""
    import torch
    from . import ops
    if metric not in ('l2', 'cosine'):
        raise ValueError("metric must be 'l2' or 'cosine' (got %r)" % (metric,))
    query_z = np.ascontiguousarray(query_z, dtype=np.float32)
    gallery_z = np.ascontiguousarray(gallery_z, dtype=np.float32)
    if query_z.ndim != 2 or gallery_z.ndim != 2 or query_z.shape[1] != gallery_z.shape[1]:
        raise ValueError("query_z (Q, d) and gallery_z (G, d) must share d")
    if exclude_self and exclude_rows is None:
        if len(query_z) > len(gallery_z):
            raise ValueError("exclude_self: query i must be gallery row i")
        exclude_rows = np.arange(len(query_z))
    if exclude_rows is not None:
        exclude_rows = np.ascontiguousarray(exclude_rows, dtype=np.int32).reshape(-1)
        if len(exclude_rows) != len(query_z):
            raise ValueError("exclude_rows needs one gallery row (or -1) per query")
    Q, k, query_block = len(query_z), int(k), max(1, int(query_block))
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    gallery = torch.from_numpy(gallery_z).to(device)
    if metric == 'cosine':
        gallery = ops.row_normalize(gallery)                      # once, not once per block
    idx = np.empty((Q, k), dtype=np.int32)
    dist = np.empty((Q, k), dtype=np.float32)
    for i in range(0, Q, query_block):
        q = torch.from_numpy(query_z[i:i + query_block]).to(device)
        if metric == 'cosine':
            q = ops.row_normalize(q)
        excl = torch.from_numpy(exclude_rows[i:i + len(q)]).to(device) if exclude_rows is not None else None
        bi, bd = ops.knn_topk(q, gallery, k, exclude=excl, metric='l2')
        idx[i:i + len(q)] = bi.cpu().numpy()
        dist[i:i + len(q)] = bd.cpu().numpy()
    return idx, dist


def average_precision_at_k(relevant, n_relevant):
    """relevant: bool (Q, k), rank j of query q is a relevant row; n_relevant: (Q,) relevant rows in the whole gallery.
    -> float64 (Q,) AP@k; NaN where n_relevant is 0 (such a query has no defined score)."""
    rel = np.asarray(relevant, dtype=bool)
    R = np.asarray(n_relevant, dtype=np.int64).reshape(-1)
    if rel.ndim != 2 or R.shape[0] != rel.shape[0]:
        raise ValueError("relevant must be (Q, k) and n_relevant (Q,)")
    k = rel.shape[1]
    hits = np.cumsum(rel, axis=1, dtype=np.float64)
    prec = hits / np.arange(1, k + 1, dtype=np.float64)
    total = np.sum(np.where(rel, prec, 0.0), axis=1)
    denom = np.minimum(k, R).astype(np.float64)
    ap = np.full(rel.shape[0], np.nan)
    ok = R > 0
    ap[ok] = total[ok] / denom[ok]
    return ap


def retrieval_scores(indices, query_y, gallery_y, exclude_self=False):
    """Scores of a ranking ``indices`` (Q, k) of gallery rows: map_at_k (mean AP@k over the queries that have a relevant row),
    precision_at_k (mean share of relevant rows among the k), recall_at_1 (the nearest row is relevant), per_class_ap
    ({label: mean AP@k of the scored queries with that label}), n_queries_scored."""
    indices = np.asarray(indices)
    query_y = np.asarray(query_y).reshape(-1)
    gallery_y = np.asarray(gallery_y).reshape(-1)
    if indices.ndim != 2 or indices.shape[0] != query_y.shape[0]:
        raise ValueError("indices must be (Q, k) with one row per query label")
    rel = gallery_y[indices] == query_y[:, None]
    labels, counts = np.unique(gallery_y, return_counts=True)
    pos = np.searchsorted(labels, query_y)
    pos_c = np.minimum(pos, len(labels) - 1)
    R = np.where(labels[pos_c] == query_y, counts[pos_c], 0).astype(np.int64)
    if exclude_self:
        R = np.maximum(R - 1, 0)
    ap = average_precision_at_k(rel, R)
    scored = R > 0
    n = int(scored.sum())
    per_class = {}
    for c in np.unique(query_y[scored]):
        per_class[c.item() if hasattr(c, 'item') else c] = float(ap[scored & (query_y == c)].mean())
    return {
        'map_at_k': float(ap[scored].mean()) if n else 0.0,
        'precision_at_k': float(rel[scored].mean()) if n else 0.0,
        'recall_at_1': float(rel[scored, 0].mean()) if n else 0.0,
        'per_class_ap': per_class,
        'n_queries_scored': n,
    }
