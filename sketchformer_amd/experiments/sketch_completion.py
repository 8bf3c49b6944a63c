"""sketch-completion: how well the model finishes a sketch somebody has started.  For the first n_sketches of a split and every
fraction in ``fractions`` the sketch is cut after that share of its tokens and closed with EOS, and the decoder continues the cut
part (model.complete: prefix-forced decoding, include/skf.h).  source=partial takes the embedding from the cut sketch - the honest
test of an embedding computed from a partial drawing; source=full takes it from the whole sketch, the upper bound.  Per fraction:
the token error rate of the completion against the original (align.token_edit_distance, normalised), the normalised DTW between
their pen positions (align.sketch_dtw), the class accuracy from the partial's embedding and the class accuracy after re-encoding
the completion.  The reference decodes from the start symbol only and ships no such experiment.  Writes one .npz and prints the
table.  The cutting and the aggregation are plain functions of host arrays."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..utils import hparams as hp


def cut_sketches(x, fraction, sos, eos):
    """Model-ready token rows ``[SOS] body [EOS] PAD...`` (n, L) cut after ``fraction`` of their body: ``(partial, kept, body_len)``.
    body_len (n,): the tokens behind a leading SOS and in front of the first EOS or PAD - to the row's end for a truncated row
    without EOS; kept = floor(fraction * body_len + 1/2); partial (n, L): the row's start with its first ``kept`` body tokens, EOS
    behind them, PAD to the end.  A row whose kept part fills all L columns stays as it is: no EOS fits behind it."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("x must be (n, L) token rows (got shape %r)" % (tuple(x.shape),))
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("fraction must be in [0, 1] (got %r)" % (fraction,))
    n, L = x.shape
    partial = np.zeros_like(x)
    kept = np.zeros(n, dtype=np.int32)
    body_len = np.zeros(n, dtype=np.int32)
    for i in range(n):
        start = 1 if L and x[i, 0] == sos else 0
        body = x[i, start:]
        stop = np.nonzero((body == eos) | (body == 0))[0]
        m = int(stop[0]) if len(stop) else len(body)
        k = min(int(np.floor(float(fraction) * m + 0.5)), m)
        body_len[i], kept[i] = m, k
        partial[i, :start + k] = x[i, :start + k]
        if start + k < L:
            partial[i, start + k] = eos
    return partial, kept, body_len


def aggregate(fractions, token_error, dtw, labels, class_partial=None, class_completed=None):
    """Per-fraction means of the per-sketch figures: token_error, dtw (F, n) floats; labels (n,); class_partial, class_completed
    (F, n) predicted classes or None (a model without a class head: the accuracies are NaN).  Returns a dict of (F,) float64 arrays:
    'fraction', 'token_error_rate', 'dtw', 'class_accuracy_partial', 'class_accuracy_completed'."""
    fr = np.asarray(fractions, dtype=np.float64).reshape(-1)
    te, dw = np.asarray(token_error, dtype=np.float64), np.asarray(dtw, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1)
    if te.shape != (len(fr), len(labels)) or dw.shape != te.shape:
        raise ValueError("token_error and dtw must be (fractions, sketches) = (%d, %d)" % (len(fr), len(labels)))

    def acc(c):
        if c is None:
            return np.full(len(fr), np.nan)
        c = np.asarray(c)
        if c.shape != te.shape:
            raise ValueError("predicted classes must be (fractions, sketches)")
        return (c == labels[None, :]).mean(axis=1)
    return {'fraction': fr, 'token_error_rate': te.mean(axis=1), 'dtw': dw.mean(axis=1),
            'class_accuracy_partial': acc(class_partial), 'class_accuracy_completed': acc(class_completed)}


def format_table(table):
    lines = ["fraction  token-error  dtw       acc(partial)  acc(completed)"]
    for i in range(len(table['fraction'])):
        lines.append("%-8.3g  %-11.4f  %-8.4f  %-12.4f  %-14.4f" % tuple(
            float(table[k][i]) for k in ('fraction', 'token_error_rate', 'dtw', 'class_accuracy_partial', 'class_accuracy_completed')))
    return "\n".join(lines)


class SketchCompletion(Experiment):
    name = "sketch-completion"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(set_type='test', n_sketches=64, fractions=[0.25, 0.5, 0.75], source='partial', mode='greedy', prefill=True, beam_width=4,
                          temperature=1.0, top_k=0, top_p=1.0, seed=0, target_file='sketch_completion.npz')

    def _classes(self, model, x):
        bs = model.hps['batch_size']
        out = [model.predict_class(x[i:i + bs])['class'] for i in range(0, len(x), bs)]
        return None if out[0] is None else np.concatenate(out).astype(np.int32)

    def compute(self, model=None):
        from .. import align
        h = self.hps
        if model.dataset.hps['use_continuous_data']:
            raise ValueError("sketch-completion: a prefix is a sequence of tokens; the experiment is built for token models")
        n, source, mode = int(h['n_sketches']), str(h['source']), str(h['mode'])
        if n < 1:
            raise ValueError("sketch-completion: n_sketches must be >= 1")
        if source not in ('partial', 'full'):
            raise ValueError("sketch-completion: source must be 'partial' or 'full'")
        fractions = [float(f) for f in h['fractions']]       # (a list: --exp-hparams fractions=[0.25,0.5,0.75])
        x, y = model.dataset.get_n_samples_from(h['set_type'], n)
        x = np.asarray(x)[:n]
        if x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n, L = x.shape
        labels = np.asarray(y).reshape(-1)[:n]
        tok = model.dataset.tokenizer
        kw = dict(mode=mode, prefill=bool(h['prefill']))        # (prefill=false: one position launch per prefix token)
        if mode == 'sample':
            kw.update(n_samples=1, temperature=float(h['temperature']), top_k=int(h['top_k']), top_p=float(h['top_p']), seed=int(h['seed']))
        elif mode == 'beam':
            kw.update(beam_width=int(h['beam_width']))
        partials, kept, recons, ter, dtw, cls_p, cls_c = [], [], [], [], [], [], []
        body_len = None
        for f in fractions:
            part, k, body_len = cut_sketches(x, f, tok.SOS, tok.EOS)
            if source == 'partial':
                res = model.complete(part, **kw)
            else:
                start = (x[:, 0] == tok.SOS).astype(np.int64)
                prefix = np.stack([np.concatenate([x[i, start[i]:], np.zeros(start[i], x.dtype)]) for i in range(n)])
                tlen = None if model.hps['blind_decoder_mask'] else np.sum(x > 0, axis=-1).reshape(-1)
                res = model.complete_from_embedding(model._embed_on_device(x), prefix, prefix_len=k, expected_len=tlen, **kw)
            recon = res['recon'] if mode == 'greedy' else res['recon'][:, 0]          # the one draw / the best hypothesis
            recon = np.ascontiguousarray(recon)
            ter.append(align.token_edit_distance(recon, x, tok, normalize=True).cpu().numpy())
            dtw.append(align.sketch_dtw(recon, x, kind='tokens', tokenizer=tok, normalize=True).cpu().numpy())
            cls_p.append(self._classes(model, part))
            cls_c.append(self._classes(model, recon[:, :L].astype(x.dtype)))
            partials.append(part); kept.append(k); recons.append(recon)
        has_cls = cls_p[0] is not None
        table = aggregate(fractions, np.stack(ter), np.stack(dtw), labels, np.stack(cls_p) if has_cls else None,
                          np.stack(cls_c) if has_cls else None)
        target = h['target_file'] if os.path.isabs(h['target_file']) else os.path.join(self.out_dir, h['target_file'])
        np.savez(target, inputs=x, labels=labels, body_len=body_len, partial=np.stack(partials), kept=np.stack(kept),
                 completion=np.stack(recons), token_error=np.stack(ter), dtw_distance=np.stack(dtw),
                 class_partial=np.stack(cls_p) if has_cls else np.zeros((len(fractions), 0), np.int32),
                 class_completed=np.stack(cls_c) if has_cls else np.zeros((len(fractions), 0), np.int32),
                 source=np.array(source), mode=np.array(mode), **table)
        print("sketch-completion: %d sketches of '%s', embedding from the %s sketch, %s decoding" % (n, h['set_type'], source, mode))
        print(format_table(table))
        return target
