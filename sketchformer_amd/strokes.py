"""Stroke edits: new sketches out of the strokes of old ones - permuted, reversed, with strokes left out - through
ops.stroke_edit (skf_stroke_edit_count / _emit; the rule is in include/skf.h).  `data` is either a list of
stroke-3 arrays (n, 3), or a pair (flat (P, 3) float32, offsets (N + 1) int64) of device tensors as ops.sketch_encode takes them;
the result comes back as the same kind.  The selection lists are built in numpy from the stroke counts - the builders below are
plain functions of those counts - and the rows are moved on the device."""
import numpy as np

from .preprocess import pack_ragged


def _is_device_pair(data):
    return isinstance(data, tuple) and len(data) == 2 and hasattr(data[0], "is_cuda")


def _on_device(data):
    """-> (flat, offsets) device tensors, N"""
    import torch
    if _is_device_pair(data):
        return data[0], data[1], data[1].shape[0] - 1
    flat, offsets = pack_ragged(data)
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), len(data)


def stroke_counts(data, return_table=False):
    """The number of strokes of every sketch, int64 (N,): a stroke ends at a row with pen == 1 or at the sketch's last row; an empty
    sketch has none.  Lists are counted on the host, a device pair through ops.stroke_table (return_table: also that table)."""
    if _is_device_pair(data):
        from . import ops
        table = ops.stroke_table(data[0], data[1])
        counts = np.diff(table[0].cpu().numpy())
        return (counts, table) if return_table else counts
    counts = np.zeros(len(data), np.int64)
    for i, s in enumerate(data):
        s = np.asarray(s)
        if len(s):
            counts[i] = int(np.count_nonzero(s[:-1, 2] == 1)) + 1
    return (counts, None) if return_table else counts


def pack_selections(selections):
    """list of M selection lists -> (sel int32 (Q,), sel_offsets int64 (M + 1))"""
    lens = np.fromiter((len(l) for l in selections), dtype=np.int64, count=len(selections))
    sel_offsets = np.zeros(len(selections) + 1, dtype=np.int64)
    np.cumsum(lens, out=sel_offsets[1:])
    if sel_offsets[-1] >= 1 << 31:
        raise ValueError("an edit lists fewer than 2^31 strokes")
    sel = np.zeros(int(sel_offsets[-1]), dtype=np.int32)
    for l, o in zip(selections, sel_offsets[:-1]):
        sel[o:o + len(l)] = np.asarray(l, dtype=np.int64).reshape(-1)
    return sel, sel_offsets


# ---------------------------------------------------------------- list builders: plain numpy over the stroke counts
def identity_lists(counts):
    return [np.arange(int(c), dtype=np.int32) for c in counts]


def permutation_lists(counts, orders=None, seed=None):
    """Every sketch's strokes in another order.  orders: one permutation per sketch; None draws them, one
    np.random.RandomState(seed).permutation per sketch in sketch order."""
    if orders is None:
        rng = np.random.RandomState(seed)
        return [rng.permutation(int(c)).astype(np.int32) for c in counts]
    if len(orders) != len(counts):
        raise ValueError("orders must hold one permutation per sketch")
    out = []
    for c, o in zip(counts, orders):
        o = np.asarray(o, dtype=np.int64).reshape(-1)
        if not np.array_equal(np.sort(o), np.arange(int(c))):
            raise ValueError("an order must be a permutation of the sketch's %d strokes (got %r)" % (int(c), o.tolist()))
        out.append(o.astype(np.int32))
    return out


def reverse_lists(counts, direction=True, order=False):
    """direction: every stroke drawn backwards (~k); order: the strokes in reverse order.  Both: the sketch backwards in time."""
    out = []
    for c in counts:
        k = np.arange(int(c), dtype=np.int32)
        if order:
            k = k[::-1]
        out.append(np.ascontiguousarray(~k if direction else k))
    return out


def keep_first_lists(counts, k):
    if int(k) < 0:
        raise ValueError("k must not be negative")
    return [np.arange(min(int(c), int(k)), dtype=np.int32) for c in counts]


def leave_one_out_lists(counts):
    """-> (lists, owner int32 (V,), dropped int32 (V,)): for every sketch of two strokes or more and every stroke j of it, the
    sketch without stroke j; sketch after sketch, j ascending.  A sketch of one stroke gives no variant (nothing would be left)."""
    lists, owner, dropped = [], [], []
    for i, c in enumerate(counts):
        c = int(c)
        if c < 2:
            continue
        k = np.arange(c, dtype=np.int32)
        for j in range(c):
            lists.append(np.ascontiguousarray(k[k != j]))
            owner.append(i)
            dropped.append(j)
    return lists, np.array(owner, np.int32), np.array(dropped, np.int32)


# ---------------------------------------------------------------- the edits
def edit(data, src, selections, table=None):
    """M output sketches: output m is built from the strokes selections[m] of sketch src[m] (k >= 0: stroke k as stored, ~k: drawn
    backwards; an entry that names no stroke gives no rows).  -> the same kind as data: a list of M float32 (n', 3) arrays, or
    (out_flat, out_offsets) device tensors.  table: ops.stroke_table of a device pair, when the caller has it."""
    import torch
    from . import ops
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    if len(src) != len(selections) or len(src) == 0:
        raise ValueError("edit needs one selection list per output sketch, and at least one")
    if src.min() < -(1 << 31) or src.max() >= 1 << 31:
        raise ValueError("src must fit 32 bits")
    sel, sel_offsets = pack_selections(selections)
    flat, offsets, _ = _on_device(data)
    if flat.shape[0] == 0:                                       # only empty sketches: every entry is absent
        out = (torch.zeros(0, 3, dtype=torch.float32, device=flat.device), torch.zeros(len(src) + 1, dtype=torch.int64, device=flat.device))
    else:
        dev = flat.device
        out = ops.stroke_edit(flat, offsets, torch.from_numpy(src.astype(np.int32)).to(dev), torch.from_numpy(sel_offsets).to(dev),
                              torch.from_numpy(sel).to(dev), table=table)
    if _is_device_pair(data):
        return out
    rows, off = out[0].cpu().numpy(), out[1].cpu().numpy()
    return [rows[off[m]:off[m + 1]] for m in range(len(src))]


def _edit_all(data, builder):
    counts, table = stroke_counts(data, return_table=True)
    return edit(data, np.arange(len(counts)), builder(counts), table=table)


def permute_strokes(data, orders=None, seed=None):
    """Every sketch with its strokes in another order, the ink unchanged (permutation_lists)."""
    return _edit_all(data, lambda c: permutation_lists(c, orders, seed))


def reverse_strokes(data, direction=True, order=False):
    """Every stroke drawn backwards; with order=True the strokes also come in reverse order: the sketch drawn exactly backwards in
    time.  direction=False, order=True reverses the order alone."""
    return _edit_all(data, lambda c: reverse_lists(c, direction, order))


def keep_first_strokes(data, k):
    """The first k strokes of every sketch (all of a sketch that has fewer)."""
    return _edit_all(data, lambda c: keep_first_lists(c, k))


def leave_one_stroke_out(data):
    """-> (variants, owner, dropped): for every sketch of two strokes or more, the sketch without its stroke j, for every j
    (leave_one_out_lists).  An empty sketch is refused, as preprocess.encode_chunk refuses one: it cannot be encoded."""
    counts, table = stroke_counts(data, return_table=True)
    if len(counts) and counts.min() == 0:
        raise IndexError("empty sketch")
    lists, owner, dropped = leave_one_out_lists(counts)
    if not lists:
        raise ValueError("leave_one_stroke_out: no sketch has two strokes or more")
    return edit(data, owner, lists, table=table), owner, dropped
