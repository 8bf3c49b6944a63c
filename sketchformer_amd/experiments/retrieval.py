"""sketch-retrieval: rank the embeddings of one split against those of another with the exact device k-NN search and score the
ranking by class label (mAP@k, precision@k, recall@1).  The reference's README claims retrieval for the embedding and ships no
experiment for it; this one embeds the way extract-embeddings does (model.predict_class) and saves one .npz."""
import os

import numpy as np

from .. import retrieval
from ..core.experiments import Experiment
from ..utils import hparams as hp


class SketchRetrieval(Experiment):
    name = "sketch-retrieval"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(batch_size=256, gallery_set='test', query_set='valid', top_k=100, metric='l2', n_queries=0,
                          target_file='retrieval.npz')

    @staticmethod
    def _embed(model, set_type, bs):
        all_x, all_y = model.dataset.get_all_data_from(set_type)
        z = [model.predict_class(all_x[i:i + bs])['embedding'] for i in range(0, len(all_x), bs)]
        return np.concatenate(z, axis=0).astype(np.float32), np.asarray(all_y).reshape(-1)

    def compute(self, model=None):
        bs = min(self.hps['batch_size'], model.hps['batch_size'])          # the engine's batch is its capacity per call
        same = self.hps['gallery_set'] == self.hps['query_set']
        gallery_z, gallery_y = self._embed(model, self.hps['gallery_set'], bs)
        query_z, query_y = (gallery_z, gallery_y) if same else self._embed(model, self.hps['query_set'], bs)
        k = max(1, min(int(self.hps['top_k']), 128, len(gallery_z) - (1 if same else 0)))
        n = int(self.hps['n_queries'])
        if 0 < n < len(query_z):
            chosen = np.sort(np.random.RandomState(14).choice(len(query_z), size=n, replace=False))
        else:
            chosen = np.arange(len(query_z))
        # one split on both sides: leave-one-out, query j is gallery row chosen[j]
        idx, dist = retrieval.retrieve(query_z[chosen], gallery_z, k, metric=self.hps['metric'],
                                       exclude_rows=chosen if same else None)
        query_y = query_y[chosen]
        scores = retrieval.retrieval_scores(idx, query_y, gallery_y, exclude_self=same)
        names = np.asarray(getattr(model.dataset, 'class_names', np.arange(int(gallery_y.max()) + 1)))
        per_class = np.full(len(names), np.nan)
        for c, ap in scores['per_class_ap'].items():
            if 0 <= int(c) < len(per_class):
                per_class[int(c)] = ap
        target = self.hps['target_file']
        if not os.path.isabs(target):
            target = os.path.join(self.out_dir, target)
        np.savez(target, indices=idx, distances=dist, query_y=query_y, gallery_y=gallery_y, query_rows=chosen,
                 map_at_k=scores['map_at_k'], precision_at_k=scores['precision_at_k'], recall_at_1=scores['recall_at_1'],
                 per_class_ap=per_class, class_names=names)
        return target
