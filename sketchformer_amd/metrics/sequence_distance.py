"""recon-token-error and recon-dtw: reconstruction quality measured on what the model emits - an ordered sequence - instead of
on its picture.  The 32 seeded validation sketches of the evaluation mixin are aligned with their greedy reconstructions on the
device (sketchformer_amd/align.py): token rows by the unit-cost edit distance divided by the longer length (the token error
rate), pen positions by dynamic time warping divided by the sum of the two lengths.  Two drawings with the same ink and another
stroke order score a raster IoU of 1 and a large distance here.  The reference has no such metric (metrics/samples.py)."""
import numpy as np

from ..core.metrics import HistoryMetric


def _pairs(input_data, name):
    x, y, pred_x, pred_y, pred_z, tokenizer, plot_filepath, tmp_filepath, is_continuous = input_data
    x, pred_x = np.asarray(x), np.asarray(pred_x)
    n = min(len(x), len(pred_x))
    if n < 1:
        raise ValueError("%s needs reconstructions (do_reconstruction)" % name)
    return x[:n], pred_x[:n], tokenizer, is_continuous


class ReconstructionTokenError(HistoryMetric):
    name = 'recon-token-error'
    input_type = 'predictions_on_validation_set'

    def compute(self, input_data):
        from .. import align
        x, recon, tokenizer, is_continuous = _pairs(input_data, self.name)
        if is_continuous:
            raise ValueError("recon-token-error compares token ids: a continuous (stroke-5) model has none; use recon-dtw")
        return float(align.token_edit_distance(x, recon, tokenizer, normalize=True).mean().cpu())


class ReconstructionDTW(HistoryMetric):
    name = 'recon-dtw'
    input_type = 'predictions_on_validation_set'

    def compute(self, input_data):
        from .. import align
        x, recon, tokenizer, is_continuous = _pairs(input_data, self.name)
        if is_continuous:
            d = align.sketch_dtw(x, recon[:, 1:], kind='stroke5')         # row 0 of a reconstruction = start symbol
        else:
            d = align.sketch_dtw(x, recon, kind='tokens', tokenizer=tokenizer)
        return float(d.mean().cpu())
