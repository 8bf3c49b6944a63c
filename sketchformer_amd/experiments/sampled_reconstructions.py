"""sampled-reconstructions: what the bottleneck of a sketch encodes, shown as variations.  For the first n_sketches of a split
the decoder draws n_samples reconstructions per sketch (model.sample: temperature, top-k and nucleus decoding on the device)
next to the greedy one.  The reference decodes by argmax only and ships no such experiment.  Writes one .npz (inputs, greedy
reconstruction, samples, parameters) and one PNG grid, a row per sketch: original, greedy, samples."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..metrics.samples import strokes_to_lines
from ..utils import hparams as hp


def write_grid_png(rows, path, colors=("k", "tab:blue", "tab:orange")):
    """rows: lists of stroke-3 sketches, one list per grid row (original, greedy, samples...); drawn like the
    sketch-reconstruction grid of metrics/samples.py.  colors: original, greedy, every sample."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    n_rows, n_cols = max(len(rows), 1), max(max((len(r) for r in rows), default=1), 1)
    fig, axes = plt.subplots(n_rows, n_cols, figsize=(2 * n_cols, 2 * n_rows), squeeze=False)
    for i in range(n_rows):
        for k in range(n_cols):
            ax = axes[i][k]
            ax.axis("off")
            if i < len(rows) and k < len(rows[i]):
                s = np.nan_to_num(np.asarray(rows[i][k], dtype=np.float64).reshape(-1, 3), posinf=0.0, neginf=0.0)
                for ln in (strokes_to_lines(s) if len(s) else []):
                    ax.plot(ln[:, 0], -ln[:, 1], color=colors[min(k, 2)], linewidth=1)
                ax.set_aspect("equal")
    fig.savefig(path, dpi=60)
    plt.close(fig)
    return path


class SampledReconstructions(Experiment):
    name = "sampled-reconstructions"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(set_type='valid', n_sketches=8, n_samples=6, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                          target_file='sampled_reconstructions.npz', plot_file='sampled_reconstructions.png')

    def _path(self, key):
        p = self.hps[key]
        return p if os.path.isabs(p) else os.path.join(self.out_dir, p)

    def compute(self, model=None):
        h = self.hps
        if model.dataset.hps['use_continuous_data']:
            raise ValueError("sampled-reconstructions: sampled decoding is built for token models")
        n, S = int(h['n_sketches']), int(h['n_samples'])
        if n < 1 or S < 1:
            raise ValueError("sampled-reconstructions: n_sketches and n_samples must be >= 1")
        x, y = model.dataset.get_n_samples_from(h['set_type'], n)
        x = np.asarray(x)[:n]
        if x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n = len(x)
        bs = model.hps['batch_size']                                     # the engine's batch is its capacity per call
        greedy = np.zeros((n, model.seq_len + 1), dtype=np.int32)
        for i in range(0, n, bs):
            r = model.predict(x[i:i + bs])['recon']
            greedy[i:i + len(r), :r.shape[1]] = r
        res = model.sample(x, n_samples=S, temperature=float(h['temperature']), top_k=int(h['top_k']), top_p=float(h['top_p']),
                           seed=int(h['seed']))
        samples = res['recon']                                           # (n, S, seq_len + 1)
        tok = model.dataset.tokenizer
        rows = [[tok.decode_single(x[i]), tok.decode_single(greedy[i])] + [tok.decode_single(s) for s in samples[i]]
                for i in range(n)]
        plot = write_grid_png(rows, self._path('plot_file'))
        target = self._path('target_file')
        np.savez(target, inputs=x, labels=np.asarray(y).reshape(-1)[:n], greedy=greedy, samples=samples,
                 temperature=np.float32(h['temperature']), top_k=np.int32(h['top_k']), top_p=np.float32(h['top_p']),
                 seed=np.int64(h['seed']), n_samples=np.int32(S), plot=np.array(os.path.basename(plot)))
        return target
