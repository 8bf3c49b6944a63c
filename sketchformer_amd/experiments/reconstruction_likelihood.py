"""reconstruction-likelihood: how well the model explains sketches, per sketch.  The first n_sketches of a split are scored
teacher-forced against themselves (model.score: the forward, then one read-once kernel over its logits): per-sketch
log-likelihood, scored length and perplexity, the corpus perplexity exp(-sum logp / sum length), top-1 / top-k position accuracy
(the share of scored positions whose target ranks below k), the mean negative log-likelihood per token of every class, and the 16
sketches the model explains worst.  With n_samples > 0 the sampled reconstructions of every sketch are scored given the sketch and
stored best first, next to the greedy reconstruction's score; with beam_width > 0 the beam's own score of every hypothesis is
stored next to its teacher-forced score - a standing self-check of the two code paths.  The reference has no scoring and ships no
such experiment.  Writes one .npz and prints one summary line."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..utils import hparams as hp

N_WORST = 16


class ReconstructionLikelihood(Experiment):
    name = "reconstruction-likelihood"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(set_type='valid', n_sketches=256, top_k=5, n_samples=0, beam_width=0, temperature=1.0, top_p=1.0, seed=0,
                          target_file='reconstruction_likelihood.npz')

    def compute(self, model=None):
        h = self.hps
        if model.dataset.hps['use_continuous_data']:
            raise ValueError("reconstruction-likelihood: teacher-forced scoring is built for token models")
        n, k, S, W = int(h['n_sketches']), int(h['top_k']), int(h['n_samples']), int(h['beam_width'])
        if n < 1 or k < 1 or S < 0 or W < 0:
            raise ValueError("reconstruction-likelihood: n_sketches and top_k must be >= 1, n_samples and beam_width >= 0")
        x, y = model.dataset.get_n_samples_from(h['set_type'], n)
        x = np.asarray(x)[:n]
        if x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n = len(x)
        labels = np.asarray(y).reshape(-1)[:n]
        res = model.score(x)
        logp, length, rank = res['logp'].astype(np.float64), res['length'].astype(np.int64), res['rank']
        scored = rank >= 0
        n_scored = max(int(scored.sum()), 1)
        classes = np.unique(labels)
        out = dict(
            inputs=x, labels=labels, logp=res['logp'], length=res['length'], perplexity=res['perplexity'], complete=res['complete'],
            corpus_perplexity=np.float64(np.exp(-logp.sum() / max(int(length.sum()), 1))),
            top1_accuracy=np.float64((scored & (rank < 1)).sum() / n_scored),
            topk_accuracy=np.float64((scored & (rank < k)).sum() / n_scored), top_k=np.int32(k),
            classes=classes,
            class_nll=np.array([-logp[labels == c].sum() / max(int(length[labels == c].sum()), 1) for c in classes], np.float64),
            worst=np.argsort(-(-logp / np.maximum(length, 1)), kind="stable")[:N_WORST].astype(np.int64))
        line = ("reconstruction-likelihood: %d sketches, corpus perplexity %.4f, top-1 accuracy %.4f, top-%d accuracy %.4f"
                % (n, float(out['corpus_perplexity']), float(out['top1_accuracy']), k, float(out['topk_accuracy'])))
        if S > 0:
            bs = model.hps['batch_size']                                 # predict takes at most a batch per call
            greedy = np.zeros((n, model.seq_len + 1), dtype=np.int32)
            for i in range(0, n, bs):
                r = model.predict(x[i:i + bs])['recon']
                greedy[i:i + len(r), :r.shape[1]] = r
            samples = model.sample(x, n_samples=S, temperature=float(h['temperature']), top_p=float(h['top_p']),
                                   seed=int(h['seed']))['recon']          # (n, S, seq_len + 1)
            sc = model.score(np.repeat(x, S, axis=0), samples.reshape(n * S, -1))
            s_logp, s_len = sc['logp'].reshape(n, S), sc['length'].reshape(n, S)
            order = np.argsort(-s_logp, axis=1, kind="stable")            # best first
            out.update(samples=np.take_along_axis(samples, order[:, :, None], axis=1), sample_logp=np.take_along_axis(s_logp, order, axis=1),
                       sample_length=np.take_along_axis(s_len, order, axis=1), greedy=greedy, greedy_logp=model.score(x, greedy)['logp'],
                       temperature=np.float32(h['temperature']), top_p=np.float32(h['top_p']), seed=np.int64(h['seed']))
            line += ", mean log-likelihood greedy %.4f, best of %d samples %.4f" % (float(out['greedy_logp'].mean()), S,
                                                                                    float(out['sample_logp'][:, 0].mean()))
        if W > 0:
            beams = model.beam_search(x, beam_width=W)
            sc = model.score(np.repeat(x, W, axis=0), beams['recon'].reshape(n * W, -1))
            out.update(beams=beams['recon'], beam_score=beams['score'], beam_length=beams['length'], beam_logp=sc['logp'].reshape(n, W),
                       beam_scored_length=sc['length'].reshape(n, W))
            # (a hypothesis without EOS that holds a PAD is scored to that PAD only: the pair is comparable where the lengths agree)
            same = out['beam_length'] == out['beam_scored_length']
            diff = np.abs(out['beam_score'].astype(np.float64) - out['beam_logp'])[same]
            line += ", beam score against teacher-forced score: largest difference %.3g over %d of %d hypotheses" % (
                float(diff.max()) if diff.size else 0.0, int(same.sum()), same.size)
        p = h['target_file']
        target = p if os.path.isabs(p) else os.path.join(self.out_dir, p)
        np.savez(target, **out)
        print(line)
        return target
