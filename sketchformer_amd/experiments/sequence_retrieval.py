"""sequence-retrieval: the classical baselines of sketch retrieval - rank the sketches of one split against those of another by
a distance between the drawings themselves and score the ranking by class label exactly as sketch-retrieval scores the learned
embedding (mAP@k, precision@k, recall@1).  distance=edit / dtw: an alignment distance between the sequences, the token edit
distance or dynamic time warping over the pen positions, one dynamic program per (query, gallery) pair.  distance=chamfer /
hausdorff: an order-free distance between the ink, the mean or the worst nearest-ink distance with samples_per_segment samples
per segment, every sketch centred on its bounding box first (a sketch starts at its first pen position).  resample_points=n
(distance=dtw only; 0 = off) resamples every sketch's pen path to n points equally spaced along it before the alignment, so that
the vertex density of a drawing plays no part.  All on the device
(sketchformer_amd/align.py); the gallery walks through in blocks so the distance matrix is built a slab at a time.  Uses
model.dataset only; writes one .npz with the keys of retrieval.npz."""
import os

import numpy as np

from .. import retrieval
from ..core.experiments import Experiment
from ..utils import hparams as hp


class SequenceRetrieval(Experiment):
    name = "sequence-retrieval"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(distance='dtw', gallery_set='test', query_set='valid', top_k=100, n_queries=256, n_gallery=4096,
                          gallery_block=1024, target_file='sequence_retrieval.npz', samples_per_segment=4, resample_points=0)

    @staticmethod
    def _subsample(n_rows, n):
        """n seeded rows of n_rows, ascending (0 = all)"""
        if 0 < n < n_rows:
            return np.sort(np.random.RandomState(14).choice(n_rows, size=n, replace=False))
        return np.arange(n_rows)

    def compute(self, model=None):
        import torch
        from .. import align
        h = self.hps
        if h['distance'] not in ('edit', 'dtw', 'chamfer', 'hausdorff'):
            raise ValueError("sequence-retrieval: distance must be 'edit', 'dtw', 'chamfer' or 'hausdorff' (got %r)" % (h['distance'],))
        continuous = bool(model.dataset.hps['use_continuous_data'])
        if continuous and h['distance'] == 'edit':
            raise ValueError("sequence-retrieval: distance=edit compares token ids; a continuous (stroke-5) dataset has none")
        tokenizer = None if continuous else model.dataset.tokenizer
        same = h['gallery_set'] == h['query_set']

        def load(set_type):
            x, y = model.dataset.get_all_data_from(set_type)
            x = np.asarray(x)
            if not continuous and x.ndim == 3:
                x = np.squeeze(x, axis=-1)                                # (N, L, 1) token columns of the file loaders
            return x, np.asarray(y).reshape(-1)

        gallery_x, gallery_y = load(h['gallery_set'])
        query_x, query_y = (gallery_x, gallery_y) if same else load(h['query_set'])
        gallery_rows = self._subsample(len(gallery_x), int(h['n_gallery']))
        gallery_x, gallery_y = gallery_x[gallery_rows], gallery_y[gallery_rows]
        if same:                                                          # the queries are drawn from the gallery that is ranked
            chosen = self._subsample(len(gallery_x), int(h['n_queries']))
            query_x, query_y, query_rows = gallery_x[chosen], gallery_y[chosen], gallery_rows[chosen]
        else:
            chosen = query_rows = self._subsample(len(query_x), int(h['n_queries']))
            query_x, query_y = query_x[chosen], query_y[chosen]
        block = max(1, int(h['gallery_block']))
        kind = dict(kind='stroke5') if continuous else dict(kind='tokens', tokenizer=tokenizer)
        slabs = []
        for at in range(0, len(gallery_x), block):
            g = gallery_x[at:at + block]
            if h['distance'] == 'edit':
                slabs.append(align.token_edit_distance(query_x, g, tokenizer, cross=True).to(torch.float32))
            elif h['distance'] in ('chamfer', 'hausdorff'):
                fn = align.sketch_chamfer if h['distance'] == 'chamfer' else align.sketch_hausdorff
                slabs.append(fn(query_x, g, cross=True, samples_per_segment=int(h['samples_per_segment']), center=True, **kind))
            else:
                slabs.append(align.sketch_dtw(query_x, g, cross=True, normalize=False, resample=int(h['resample_points']) or None, **kind))
        D = torch.cat(slabs, dim=1)
        k = max(1, min(int(h['top_k']), len(gallery_x) - (1 if same else 0)))
        # one split on both sides: leave-one-out, query j is gallery row chosen[j]
        idx, dist = align.rank_by_distance(D, k, exclude_rows=chosen if same else None)
        scores = retrieval.retrieval_scores(idx, query_y, gallery_y, exclude_self=same)
        names = np.asarray(getattr(model.dataset, 'class_names', np.arange(int(gallery_y.max()) + 1)))
        per_class = np.full(len(names), np.nan)
        for c, ap in scores['per_class_ap'].items():
            if 0 <= int(c) < len(per_class):
                per_class[int(c)] = ap
        target = h['target_file']
        if not os.path.isabs(target):
            target = os.path.join(self.out_dir, target)
        np.savez(target, indices=idx, distances=dist.astype(np.float32), query_y=query_y, gallery_y=gallery_y, query_rows=query_rows,
                 gallery_rows=gallery_rows, map_at_k=scores['map_at_k'], precision_at_k=scores['precision_at_k'],
                 recall_at_1=scores['recall_at_1'], per_class_ap=per_class, class_names=names, distance=np.array(h['distance']))
        return target
