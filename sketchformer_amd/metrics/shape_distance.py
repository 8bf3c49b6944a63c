"""recon-chamfer and recon-hausdorff: reconstruction quality measured on the ink itself.  The 32 seeded validation sketches of the
evaluation mixin are compared with their greedy reconstructions by the mean (Chamfer) and the worst (Hausdorff) distance from
the ink of one drawing to the nearest ink of the other, both ways, on the device (sketchformer_amd/align.py).  Unlike
recon-token-error and recon-dtw they do not see the order or the direction of the strokes; unlike recon-raster-iou they have no
resolution and no line width, and a reconstruction that is slightly off scores slightly worse, not zero.  Original and
reconstruction share a frame, so nothing is centred.  The reference has no such metric (metrics/samples.py)."""
from ..core.metrics import HistoryMetric
from .sequence_distance import _pairs


def _shape_distance(fn, input_data, name):
    x, recon, tokenizer, is_continuous = _pairs(input_data, name)
    if is_continuous:
        d = fn(x, recon[:, 1:], kind='stroke5')                       # row 0 of a reconstruction = start symbol
    else:
        d = fn(x, recon, kind='tokens', tokenizer=tokenizer)
    return float(d.mean().cpu())


class ReconstructionChamfer(HistoryMetric):
    name = 'recon-chamfer'
    input_type = 'predictions_on_validation_set'

    def compute(self, input_data):
        from .. import align
        return _shape_distance(align.sketch_chamfer, input_data, self.name)


class ReconstructionHausdorff(HistoryMetric):
    name = 'recon-hausdorff'
    input_type = 'predictions_on_validation_set'

    def compute(self, input_data):
        from .. import align
        return _shape_distance(align.sketch_hausdorff, input_data, self.name)
