"""stroke-sensitivity: what a trained model makes of the ORDER, the DIRECTION and the PRESENCE of strokes.  The first n_sketches
of a split are brought back to stroke-3 with the host code that draws them (the tokenizer's decode_single, or stroke5_to_stroke3
for continuous data), edited on the device (strokes / ops.stroke_edit; the rule is in include/skf.h), re-encoded on the device
under the loader's hparams (ops.sketch_encode) and run through the encoder.  The control is the identity edit through the same
route, so every comparison is like with like.  Variants:
  permutation  n_permutations random stroke orders per sketch (np.random.RandomState(seed + p), one permutation per sketch)
  direction    every stroke drawn backwards
  time         the whole drawing backwards in time (strokes reversed, and in reverse order)
  leave-one-out  every sketch of two strokes or more without its stroke j, for every j
Per variant: the cosine between its embedding and the control's, the probability of the true class, whether the arg-max class
changed, and the DTW (align.sketch_dtw) and Chamfer distance (align.sketch_chamfer, one sample per segment) between the variant's
drawing and the control's - the first is sensitive to order and direction, the second blind to both.  For leave-one-out,
importance = p_true(control) - p_true(without the stroke), aggregated by the stroke's rank and by its share of the sketch's
points.  The reference has a shuffle_stroke loader option and no such experiment.  Writes one .npz and prints the tables; the
aggregation is plain functions of host arrays."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..utils import hparams as hp

KINDS = ('permutation', 'direction', 'time')
RANKS = ('first', 'second', 'third', 'later', 'last')
SHARE_EDGES = (0.0, 0.1, 0.25, 0.5, 1.0)


def cosine(a, b):
    """Row-wise cosine of two (..., E) arrays in float64; 0 where a row has no length."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1))
    return np.where(den > 0, (a * b).sum(-1) / np.where(den > 0, den, 1.0), 0.0)


def aggregate(kinds, cosine_, p_true, control_p_true, changed, dtw, chamfer):
    """Per-kind means.  kinds: K names; cosine_, p_true, changed, dtw, chamfer: K arrays, each (..., n) over the n sketches (a
    kind with several variants per sketch has leading axes); control_p_true (n,).  -> dict of (K,) arrays: 'kind', 'cosine',
    'p_true', 'p_true_drop' (control minus variant), 'class_changed', 'dtw', 'chamfer'."""
    ctrl = np.asarray(control_p_true, np.float64).reshape(-1)
    cols = (cosine_, p_true, changed, dtw, chamfer)
    if any(len(c) != len(kinds) for c in cols):
        raise ValueError("every column needs one array per kind")
    for c in cols:
        for a in c:
            if np.asarray(a).shape[-1:] != ctrl.shape:
                raise ValueError("every array must end in the sketch axis (%d)" % len(ctrl))

    def mean(col):
        return np.array([np.asarray(a, np.float64).mean() if np.asarray(a).size else np.nan for a in col])
    return {'kind': np.array(list(kinds)), 'cosine': mean(cosine_), 'p_true': mean(p_true),
            'p_true_drop': np.array([(ctrl - np.asarray(a, np.float64)).mean() if np.asarray(a).size else np.nan for a in p_true]),
            'class_changed': mean(changed), 'dtw': mean(dtw), 'chamfer': mean(chamfer)}


def aggregate_importance(dropped, stroke_count, importance, share):
    """Leave-one-stroke-out, V variants: dropped (V,) = the stroke left out, stroke_count (V,) = the strokes of its sketch,
    importance (V,), share (V,) = the stroke's share of the sketch's points.  -> dict: 'rank' (RANKS), 'rank_importance',
    'rank_count': the mean importance of strokes that are the first, second, third, a later but not the last, and the last of
    their sketch (the last stroke counts as 'last' only); 'share_edges', 'share_importance', 'share_count': by share in
    (edge[i], edge[i + 1]].  NaN where a bin is empty."""
    dropped, stroke_count = np.asarray(dropped).reshape(-1), np.asarray(stroke_count).reshape(-1)
    importance, share = np.asarray(importance, np.float64).reshape(-1), np.asarray(share, np.float64).reshape(-1)
    if not (len(dropped) == len(stroke_count) == len(importance) == len(share)):
        raise ValueError("dropped, stroke_count, importance and share must be of one length")
    last = dropped == stroke_count - 1
    masks = [~last & (dropped == 0), ~last & (dropped == 1), ~last & (dropped == 2), ~last & (dropped >= 3), last]
    edges = np.array(SHARE_EDGES)
    bins = [(share > lo) & (share <= hi) for lo, hi in zip(edges[:-1], edges[1:])]

    def mean(m):
        return importance[m].mean() if m.any() else np.nan
    return {'rank': np.array(RANKS), 'rank_importance': np.array([mean(m) for m in masks]),
            'rank_count': np.array([int(m.sum()) for m in masks]), 'share_edges': edges,
            'share_importance': np.array([mean(m) for m in bins]), 'share_count': np.array([int(m.sum()) for m in bins])}


def format_table(table, importance=None):
    lines = ["variant      cosine    p(true)   p-drop    class-changed  dtw       chamfer"]
    for i in range(len(table['kind'])):
        lines.append("%-11s  %-8.4f  %-8.4f  %-8.4f  %-13.4f  %-8.4f  %-8.4g" % ((str(table['kind'][i]),) + tuple(
            float(table[k][i]) for k in ('cosine', 'p_true', 'p_true_drop', 'class_changed', 'dtw', 'chamfer'))))
    if importance is not None:
        lines.append("stroke       importance  strokes")
        for i, r in enumerate(importance['rank']):
            lines.append("%-11s  %-10.4f  %d" % (str(r), float(importance['rank_importance'][i]), int(importance['rank_count'][i])))
        e = importance['share_edges']
        for i in range(len(e) - 1):
            lines.append("%-11s  %-10.4f  %d" % ("%g-%g%%" % (100 * e[i], 100 * e[i + 1]), float(importance['share_importance'][i]),
                                                  int(importance['share_count'][i])))
    return "\n".join(lines)


def dense_stroke3(flat, offsets):
    """(flat (P, 3), offsets (M + 1)) device tensors -> (dense (M, T, 3) float32 zero-padded, lengths (M,) int32) on the device,
    T = the longest sketch (at least 1)."""
    import torch
    M = offsets.shape[0] - 1
    lengths = offsets[1:] - offsets[:-1]
    T = max(int(lengths.max().item()), 1) if M else 1
    dense = torch.zeros(M, T, 3, dtype=torch.float32, device=flat.device)
    if flat.shape[0]:
        row = torch.arange(flat.shape[0], device=flat.device)
        sk = torch.searchsorted(offsets[1:].contiguous(), row, right=True)
        dense[sk, row - offsets[sk]] = flat
    return dense, lengths.to(torch.int32)


class StrokeSensitivity(Experiment):
    name = "stroke-sensitivity"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(set_type='test', n_sketches=64, n_permutations=4, seed=0, max_variants_per_batch=4096,
                          target_file='stroke_sensitivity.npz')

    # ---- the route every sketch takes: stroke-3 on the device -> model input -> encoder
    def _encoder(self, model):
        """-> encode(flat, offsets): model-ready rows on the device, under the loader's hparams"""
        import torch
        from .. import ops
        from ..utils.tokenizer import GridTokenizer, Tokenizer
        hps, tok = model.dataset.hps, getattr(model.dataset, 'tokenizer', None)
        L = int(hps['max_seq_len'])
        if hps['use_continuous_data']:
            return lambda flat, offsets: ops.sketch_encode(flat, offsets, 'stroke5', L)
        if isinstance(tok, GridTokenizer):
            return lambda flat, offsets: ops.sketch_encode(flat, offsets, 'grid', L, resolution=tok.resolution)
        if isinstance(tok, Tokenizer):
            centers = torch.from_numpy(np.ascontiguousarray(tok.centers, dtype=np.float64)).cuda()
            return lambda flat, offsets: ops.sketch_encode(flat, offsets, 'dict', L, centers=centers)
        raise ValueError("stroke-sensitivity: the device encoder takes continuous data, a GridTokenizer or a dictionary Tokenizer "
                         "(got %s)" % type(tok).__name__)

    def _embed(self, model, rows):
        """Model-ready rows on the device -> (embedding (V, E) float32, class probabilities (V, C) float32 or None) on the host;
        the rows go to the encoder in chunks of batch_size, device to device."""
        import torch
        eng = model.engine
        B, V = eng.cfg.batch, rows.shape[0]
        emb, cls = None, None
        for i in range(0, V, B):
            n = min(B, V - i)
            pad = torch.zeros((B,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
            if eng.cfg.continuous:
                pad[..., 4] = 1.0
            pad[:n] = rows[i:i + n]
            eng.encode(pad)
            e = eng.buffer('embedding') if model.hps['lowerdim'] else eng.buffer('enc_output').view(B, -1)
            if emb is None:
                emb = torch.empty(V, e.shape[1], dtype=torch.float32, device=e.device)
            emb[i:i + n].copy_(e[:n])
            if model._has_cls:
                c = eng.buffer('class_probs')
                if cls is None:
                    cls = torch.empty(V, c.shape[1], dtype=torch.float32, device=c.device)
                cls[i:i + n].copy_(c[:n])
        return emb.cpu().numpy(), None if cls is None else cls.cpu().numpy()

    def compute(self, model=None):
        import torch
        from .. import align, ops, strokes
        from ..metrics.samples import stroke5_to_stroke3
        h = self.hps
        n, n_perm, seed, chunk = int(h['n_sketches']), int(h['n_permutations']), int(h['seed']), int(h['max_variants_per_batch'])
        if n < 1 or n_perm < 0 or chunk < 1:
            raise ValueError("stroke-sensitivity: n_sketches >= 1, n_permutations >= 0 and max_variants_per_batch >= 1")
        encode = self._encoder(model)
        x, y = model.dataset.get_n_samples_from(h['set_type'], n)
        x = np.asarray(x)[:n]
        continuous = bool(model.dataset.hps['use_continuous_data'])
        if not continuous and x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n = len(x)
        labels = np.asarray(y).reshape(-1)[:n].astype(np.int64)
        tok = getattr(model.dataset, 'tokenizer', None)
        sketches = [np.asarray(stroke5_to_stroke3(r) if continuous else tok.decode_single(r), dtype=np.float32).reshape(-1, 3) for r in x]
        if min(len(s) for s in sketches) == 0:
            raise IndexError("empty sketch")
        if max(len(s) for s in sketches) > ops.ALIGN_MAX_LEN:
            raise ValueError("stroke-sensitivity: sketches hold at most %d points" % ops.ALIGN_MAX_LEN)
        flat, offsets, _ = strokes._on_device(sketches)
        table = ops.stroke_table(flat, offsets)
        counts = np.diff(table[0].cpu().numpy())
        stroke_len = np.diff(table[1].cpu().numpy())

        # every variant of every kind as one edit: (src, lists), cut into calls of `chunk` output sketches
        src, lists = [np.arange(n)], [strokes.identity_lists(counts)]
        for p in range(n_perm):
            src.append(np.arange(n)); lists.append(strokes.permutation_lists(counts, seed=seed + p))
        src.append(np.arange(n)); lists.append(strokes.reverse_lists(counts, direction=True, order=False))
        src.append(np.arange(n)); lists.append(strokes.reverse_lists(counts, direction=True, order=True))
        loo_lists, owner, dropped = strokes.leave_one_out_lists(counts)
        src.append(owner.astype(np.int64)); lists.append(loo_lists)
        src = np.concatenate(src)
        lists = [l for part in lists for l in part]
        V = len(src)

        control = strokes.edit((flat, offsets), src[:n], lists[:n], table=table)
        cdense, clen = dense_stroke3(*control)
        rows_out, emb, cls, dtw, chamfer = [], [], [], [], []
        for at in range(0, V, chunk):
            vflat, voffsets = strokes.edit((flat, offsets), src[at:at + chunk], lists[at:at + chunk], table=table)
            rows = encode(vflat, voffsets)
            e, c = self._embed(model, rows)
            emb.append(e); cls.append(c)
            if at < n:
                rows_out.append(rows[:n - at].cpu().numpy())
            vdense, vlen = dense_stroke3(vflat, voffsets)
            own = torch.from_numpy(src[at:at + chunk]).to(vdense.device)
            ca, la = cdense[own].contiguous(), clen[own].contiguous()
            dtw.append(align.sketch_dtw(vdense, ca, lengths_a=vlen, lengths_b=la).cpu().numpy())
            chamfer.append(align.sketch_chamfer(vdense, ca, samples_per_segment=1, lengths_a=vlen, lengths_b=la).cpu().numpy())
        emb, dtw, chamfer = np.concatenate(emb), np.concatenate(dtw).astype(np.float64), np.concatenate(chamfer)
        has_cls = cls[0] is not None
        if has_cls:
            cls = np.concatenate(cls)
            p_true = cls[np.arange(V), labels[src]].astype(np.float64)
            pred = cls.argmax(-1).astype(np.int32)
        else:
            p_true, pred = np.full(V, np.nan), np.full(V, -1, np.int32)
        cos = cosine(emb, emb[src])                                   # (rows 0 .. n - 1 are the control)
        changed = (pred != pred[src]).astype(np.float64) if has_cls else np.full(V, np.nan)

        def part(a, kind):
            lo = {'permutation': n, 'direction': n * (1 + n_perm), 'time': n * (2 + n_perm), 'loo': n * (3 + n_perm)}[kind]
            hi = {'permutation': n * (1 + n_perm), 'direction': n * (2 + n_perm), 'time': n * (3 + n_perm), 'loo': V}[kind]
            return a[lo:hi].reshape(n_perm, n) if kind == 'permutation' else a[lo:hi]
        table_ = aggregate(KINDS, [part(cos, k) for k in KINDS], [part(p_true, k) for k in KINDS], p_true[:n],
                           [part(changed, k) for k in KINDS], [part(dtw, k) for k in KINDS], [part(chamfer, k) for k in KINDS])
        first_stroke = table[0].cpu().numpy()[:-1]
        loo_share = stroke_len[first_stroke[owner] + dropped] / np.maximum(np.diff(offsets.cpu().numpy())[owner], 1)
        importance = part(p_true[src], 'loo') - part(p_true, 'loo')
        imp = aggregate_importance(dropped, counts[owner], importance, loo_share)
        out = {'inputs': x, 'labels': labels, 'stroke_count': counts, 'control_input': np.concatenate(rows_out)[:n],
               'control_embedding': emb[:n], 'control_p_true': p_true[:n], 'control_class': pred[:n],
               'loo_owner': owner, 'loo_dropped': dropped, 'loo_share': loo_share, 'loo_importance': importance,
               'loo_p_true': part(p_true, 'loo'), 'loo_cosine': part(cos, 'loo'), 'loo_dtw': part(dtw, 'loo'),
               'loo_chamfer': part(chamfer, 'loo')}
        for k in KINDS:
            out.update({k + '_cosine': part(cos, k), k + '_p_true': part(p_true, k), k + '_class_changed': part(changed, k),
                        k + '_dtw': part(dtw, k), k + '_chamfer': part(chamfer, k)})
        out.update(table_)
        out.update(imp)
        target = h['target_file'] if os.path.isabs(h['target_file']) else os.path.join(self.out_dir, h['target_file'])
        np.savez(target, **out)
        print("stroke-sensitivity: %d sketches of '%s', %d random orders each, %d leave-one-out variants" % (n, h['set_type'], n_perm, len(owner)))
        print(format_table(table_, imp))
        return target
