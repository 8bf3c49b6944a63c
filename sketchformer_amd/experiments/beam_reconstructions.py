"""beam-reconstructions: the most likely reconstructions of a sketch, ranked.  For the first n_sketches of a split the decoder
keeps the beam_width best partial sequences per sketch (model.beam_search: the beam instantiation of the one-launch decoder plus
the merge kernel) and returns them with their log-likelihoods, next to the greedy reconstruction, whose log-likelihood is the
score of a beam of width 1.  The reference decodes by argmax only and ships no such experiment.  Writes one .npz (inputs, greedy
row and score, hypotheses with scores and lengths, parameters) and prints one summary line."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..utils import hparams as hp


class BeamReconstructions(Experiment):
    name = "beam-reconstructions"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(set_type='valid', n_sketches=8, beam_width=4, length_alpha=0.0, target_file='beam_reconstructions.npz')

    def compute(self, model=None):
        h = self.hps
        if model.dataset.hps['use_continuous_data']:
            raise ValueError("beam-reconstructions: beam search is built for token models")
        n, W = int(h['n_sketches']), int(h['beam_width'])
        if n < 1:
            raise ValueError("beam-reconstructions: n_sketches must be >= 1")
        x, y = model.dataset.get_n_samples_from(h['set_type'], n)
        x = np.asarray(x)[:n]
        if x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n = len(x)
        greedy = model.beam_search(x, beam_width=1)                      # the greedy row and its log-likelihood
        beams = model.beam_search(x, beam_width=W, length_alpha=float(h['length_alpha']))
        p = h['target_file']
        target = p if os.path.isabs(p) else os.path.join(self.out_dir, p)
        np.savez(target, inputs=x, labels=np.asarray(y).reshape(-1)[:n], greedy=greedy['recon'][:, 0], greedy_score=greedy['score'][:, 0],
                 beams=beams['recon'], scores=beams['score'], lengths=beams['length'], beam_width=np.int32(W),
                 length_alpha=np.float32(h['length_alpha']))
        print("beam-reconstructions: %d sketches, beam_width %d, mean log-likelihood greedy %.4f, best beam %.4f"
              % (n, W, float(greedy['score'][:, 0].mean()), float(beams['score'].max(axis=1).mean())))
        return target
