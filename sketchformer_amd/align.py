"""Sequence alignment: what a model emits - an ordered row of tokens, or of pen positions - against its target, as an alignment
distance computed on the device (skf_align.hip through ops.edit_distance / ops.dtw_distance).  Token rows are scored by the
unit-cost Levenshtein distance (the token error rate once divided by the longer length), point rows by dynamic time warping
under the Euclidean distance.  Both are also the classical sketch-retrieval baselines: a (Q, G) matrix of either, ranked by
``rank_by_distance``, goes into retrieval.retrieval_scores like a ranking of embeddings.  The reference has neither; it looks at
reconstructions (metrics/samples.py).  DESIGN.md section 3n.

Beside them the two order-free distances between the ink of two sketches, ``sketch_chamfer`` and ``sketch_hausdorff``
(skf_chamfer.hip through ops.shape_distance): the mean and the worst distance from one drawing to the nearest ink of the other.
They do not see in which order or direction the strokes were drawn.  DESIGN.md section 3s."""
import numpy as np


def _token_rows(tokens, device=None):
    """-> int64 (B, L) tensor with a unit innermost stride; where it is, or on `device`"""
    import torch
    t = tokens if torch.is_tensor(tokens) else torch.from_numpy(np.ascontiguousarray(tokens))
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]                                             # (N, L, 1) token columns of the file loaders
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError("token rows must be (B, L) with L >= 1 (got %r)" % (tuple(t.shape),))
    if device is not None:
        t = t.to(torch.device(device))
    t = t.to(torch.int64)
    return t if t.stride(1) == 1 else t.contiguous()


def token_spans(tokens, tokenizer):
    """The content of every token row as (view, lengths): what lies behind one leading SOS, if present, and in front of the first
    EOS or PAD - or the row's end, for a truncated row without EOS.  tokens: (B, L) ids; plain torch, computed where the rows
    are (token_edit_distance puts them on the device first).  view is a strided view INTO the rows, not a copy - (B, L - 1) from
    column 1 when every row leads with SOS, the rows themselves when none does - so the kernel reads it with a row stride larger
    than its width; only a batch that mixes both gets a copy with the SOS rows shifted left.  lengths: int32 (B,)."""
    import torch
    t = _token_rows(tokens)
    B, L = t.shape
    sos = t[:, 0] == int(tokenizer.SOS)
    n_sos = int(sos.sum())
    if n_sos == B and L > 1:
        view = t[:, 1:]
    elif n_sos == 0:
        view = t
    else:                                                          # mixed (or L == 1): shift the SOS rows left by one, PAD behind
        shifted = torch.cat([t[:, 1:], torch.full((B, 1), int(tokenizer.PAD), dtype=t.dtype, device=t.device)], dim=1)
        view = torch.where(sos[:, None], shifted, t)
    stop = (view == int(tokenizer.EOS)) | (view == int(tokenizer.PAD))
    lengths = (torch.cumsum(stop.to(torch.int32), dim=1) == 0).sum(dim=1).to(torch.int32)
    return view, lengths


def token_edit_distance(a, b, tokenizer, cross=False, normalize=False):
    """Levenshtein distance between the contents (token_spans) of token rows a (Na, La) and b (Nb, Lb): int32 (Na,) for the pairs
    (a[i], b[i]), or (Na, Nb) with cross=True.  normalize: divided by max(len_a, len_b, 1), float64 - the token error rate, in
    [0, 1].  Device tensors out."""
    import torch
    from . import ops
    dev = a.device if torch.is_tensor(a) and a.is_cuda else torch.device("cuda")
    va, la = token_spans(_token_rows(a, dev), tokenizer)
    vb, lb = token_spans(_token_rows(b, dev), tokenizer)
    d = ops.edit_distance(va, vb, la, lb, cross=cross)
    if not normalize:
        return d
    longer = torch.maximum(la[:, None], lb[None, :]) if cross else torch.maximum(la, lb)
    return d.to(torch.float64) / longer.clamp(min=1).to(torch.float64)


def _resampled_rows(xy, n, n_out):
    """Point rows xy (N, T, 2) with n (N,) points each -> ((N, n_out, 2), int32 (N,) all n_out): every row's pen path resampled to
    n_out points equally spaced along its arc length (ops.polyline_resample_n).  An empty row becomes n_out rows (0, 0), the single
    point that stands for it in the alignment."""
    import torch
    from . import ops
    N, T = xy.shape[0], xy.shape[1]
    n = n.clamp(0, T).to(torch.int64)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=xy.device)
    offsets[1:] = torch.cumsum(n, 0)
    live = torch.arange(T, device=xy.device)[None, :] < n[:, None]
    packed = xy[live]                                              # (P, 2): the rows back to back, what lies behind n left out
    if packed.shape[0] == 0:
        out = torch.zeros(N, int(n_out), 2, dtype=torch.float32, device=xy.device)
    else:
        out = ops.polyline_resample_n(packed, offsets, n_out)
    return out, torch.full((N,), int(n_out), dtype=torch.int32, device=xy.device)


def sketch_dtw(a, b, kind='stroke3', tokenizer=None, cross=False, normalize=True, lengths_a=None, lengths_b=None, resample=None):
    """Dynamic time warping between the pen positions of sketches a and b, each in any form raster.points takes ('stroke3' with
    lengths_a / lengths_b or as ragged lists, 'stroke5', 'tokens' with the tokenizer): float32 (Na,) for the pairs, (Na, Nb) with
    cross=True.  An empty sketch stands for the single point (0, 0), the dummy row of the host decoders.  normalize: divided by
    max(n_a, 1) + max(n_b, 1) (an upper bound on the length of the alignment path), float64: a mean distance per step that does
    not grow with the length of the sketches.  resample=n (2 <= n <= 512): every sketch's sequence of pen positions, taken as ONE
    path - pen-up moves included, the sequence that is aligned without it - is first resampled to n points equally spaced along
    its arc length (the rule of include/skf.h, coordinates within +-2^14), so that two drawings of one curve with different vertex
    densities are close; every sketch then counts n points.  Device tensors out."""
    import torch
    from . import ops, raster
    xa, _, na, _ = raster.points(a, kind, tokenizer, lengths_a)
    xb, _, nb, _ = raster.points(b, kind, tokenizer, lengths_b, device=xa.device)
    if resample is not None:
        if not 2 <= int(resample) <= ops.ALIGN_MAX_LEN:
            raise ValueError("resample must be in [2, %d] (got %r)" % (ops.ALIGN_MAX_LEN, resample))
        xa, na = _resampled_rows(xa, na, int(resample))
        xb, nb = _resampled_rows(xb, nb, int(resample))
    d = ops.dtw_distance(xa, na, xb, nb, cross=cross)
    if not normalize:
        return d
    ca, cb = na.clamp(min=1), nb.clamp(min=1)
    steps = (ca[:, None] + cb[None, :]) if cross else (ca + cb)
    return d.to(torch.float64) / steps.to(torch.float64)


def _shape_parts(a, b, kind, tokenizer, cross, samples_per_segment, center, lengths_a, lengths_b):
    """(mean a->b, mean b->a, max a->b, max b->a) per pair (ops.shape_distance) of sketches in any form raster.points takes"""
    from . import ops, raster
    xa, pa, na, ba = raster.points(a, kind, tokenizer, lengths_a)
    xb, pb, nb, bb = raster.points(b, kind, tokenizer, lengths_b, device=xa.device)
    if center:                                                     # the bounding-box centre, float32, on the device
        xa = xa - ((ba[:, :2] + ba[:, 2:]) * 0.5)[:, None, :]
        xb = xb - ((bb[:, :2] + bb[:, 2:]) * 0.5)[:, None, :]
    return ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=samples_per_segment, cross=cross)


def sketch_chamfer(a, b, kind='stroke3', tokenizer=None, cross=False, samples_per_segment=4, center=False, lengths_a=None,
                   lengths_b=None, return_parts=False):
    """The Chamfer distance between the ink of sketches a and b, each in any form raster.points takes (as for sketch_dtw): the mean
    distance from the samples of one sketch - its points and samples_per_segment - 1 positions inside every segment - to the nearest
    dot or segment of the other, averaged over both directions.  It does not depend on the order or the direction of the strokes,
    on a resolution or on a line width.  float32 (Na,) for the pairs, (Na, Nb) with cross=True.  center: each sketch is moved so that
    the centre of its bounding box lies at the origin first (sketches start at their first pen position: retrieval needs this; an
    original and its reconstruction share a frame and do not).  return_parts: the (..., 4) tensor of ops.shape_distance instead.
    An empty sketch stands for the single point (0, 0).  Device tensors out."""
    parts = _shape_parts(a, b, kind, tokenizer, cross, samples_per_segment, center, lengths_a, lengths_b)
    return parts if return_parts else 0.5 * (parts[..., 0] + parts[..., 1])


def sketch_hausdorff(a, b, kind='stroke3', tokenizer=None, cross=False, samples_per_segment=4, center=False, lengths_a=None,
                     lengths_b=None, return_parts=False):
    """The Hausdorff distance between the ink of sketches a and b: the largest distance from a sample of one sketch to the nearest
    dot or segment of the other, over both directions.  Arguments and shapes as for sketch_chamfer."""
    import torch
    parts = _shape_parts(a, b, kind, tokenizer, cross, samples_per_segment, center, lengths_a, lengths_b)
    return parts if return_parts else torch.maximum(parts[..., 2], parts[..., 3])


def rank_by_distance(D, k, exclude_rows=None):
    """(Q, G) distances -> (indices int32 (Q, k), distances (Q, k)) of the k smallest per row, smallest first; equal distances
    come out in gallery-row order (a stable sort).  exclude_rows (Q,): the one gallery row left out of each query's ranking
    (leave-one-out; -1 = none).  k is clamped to the rows that can be ranked.  D: a tensor on any device, or an array; numpy out,
    in the layout retrieval.retrieval_scores takes."""
    import torch
    D = D if torch.is_tensor(D) else torch.from_numpy(np.ascontiguousarray(D))
    if D.dim() != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("D must be a (Q, G) matrix (got %r)" % (tuple(D.shape),))
    Q, G = D.shape
    keys = D.to(torch.float64).clone()
    if exclude_rows is not None:
        ex = torch.as_tensor(np.asarray(exclude_rows.cpu() if torch.is_tensor(exclude_rows) else exclude_rows), dtype=torch.int64).reshape(-1).to(D.device)
        if ex.shape[0] != Q or int(ex.max()) >= G:
            raise ValueError("exclude_rows needs one gallery row (or -1) per query")
        rows = torch.nonzero(ex >= 0).reshape(-1)
        keys[rows, ex[rows]] = float('inf')                        # last in its row, and cut off by the clamp of k below
        G_rank = G - 1 if len(rows) else G
    else:
        G_rank = G
    if G_rank < 1:
        raise ValueError("nothing left to rank: the gallery holds one row and it is excluded")
    k = max(1, min(int(k), G_rank))
    order = torch.sort(keys, dim=1, stable=True).indices[:, :k]
    return order.to(torch.int32).cpu().numpy(), torch.gather(D, 1, order).cpu().numpy()
