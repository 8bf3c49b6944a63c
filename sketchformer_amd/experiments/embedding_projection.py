"""embedding-projection: the 2-D map of one split's embeddings - exact t-SNE on the device, or PCA - for up to 8192 samples, where
the `tsne` metric stops at 1000.  It embeds the way extract-embeddings does (model.predict_class), saves one .npz and a scatter
plot coloured by label.  The reference has the map only as a training-time metric; this has the same relation to that metric as
sketch-retrieval has to the README's retrieval claim."""
import os

import numpy as np

from .. import projection
from ..core.experiments import Experiment
from ..utils import hparams as hp


class EmbeddingProjection(Experiment):
    name = "embedding-projection"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(batch_size=256, set_type='valid', n_samples=5000, method='tsne', perplexity=30.0, n_iter=1000,
                          init='random', target_file='projection.npz')

    @staticmethod
    def _embed(model, set_type, bs):
        all_x, all_y = model.dataset.get_all_data_from(set_type)
        out = [model.predict_class(all_x[i:i + bs]) for i in range(0, len(all_x), bs)]
        z = np.concatenate([o['embedding'] for o in out], axis=0).astype(np.float32)
        if all('class' in o for o in out):
            pred_y = np.concatenate([np.asarray(o['class']).reshape(-1) for o in out], axis=0)
        else:                                                              # a model without the classification head
            pred_y = np.full(len(z), -1, dtype=np.int32)
        return z, np.asarray(all_y).reshape(-1), pred_y

    @staticmethod
    def _plot(path, xy, labels, title):
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(figsize=(8, 8))
        ax.scatter(xy[:, 0], xy[:, 1], c=labels, cmap='tab20', s=6, linewidths=0)
        ax.set_title(title)
        ax.set_xticks([]); ax.set_yticks([])
        fig.savefig(path, dpi=120, bbox_inches='tight')
        plt.close(fig)

    def compute(self, model=None):
        method = self.hps['method']
        if method not in ('tsne', 'pca'):
            raise ValueError("method must be 'tsne' or 'pca' (got %r)" % (method,))
        bs = min(self.hps['batch_size'], model.hps['batch_size'])          # the engine's batch is its capacity per call
        z, y, pred_y = self._embed(model, self.hps['set_type'], bs)
        n = max(1, min(int(self.hps['n_samples']), projection.MAX_POINTS, len(z)))
        rows = np.sort(np.random.RandomState(14).choice(len(z), size=n, replace=False)) if n < len(z) else np.arange(len(z))
        kl = np.nan
        if method == 'tsne':
            perplexity = min(float(self.hps['perplexity']), float(n - 1))
            xy, kl = projection.tsne(z[rows], perplexity=perplexity, n_iter=int(self.hps['n_iter']), init=self.hps['init'], seed=14,
                                     return_kl=True)
        else:
            xy = projection.pca(z[rows], 2)
        names = np.asarray(getattr(model.dataset, 'class_names', np.arange(int(y.max()) + 1)))
        target = self.hps['target_file']
        if not os.path.isabs(target):
            target = os.path.join(self.out_dir, target)
        np.savez(target, projection=np.asarray(xy, dtype=np.float32), y=y[rows], pred_y=pred_y[rows], rows=rows,
                 kl_divergence=np.float64(kl), class_names=names)
        self._plot(os.path.splitext(target)[0] + '.png', xy, y[rows],
                   "%s of %d '%s' embeddings" % (method, n, self.hps['set_type']))
        return target
