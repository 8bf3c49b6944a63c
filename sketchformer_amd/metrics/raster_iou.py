"""recon-raster-iou: reconstruction quality as a number.  The 32 seeded validation sketches of the evaluation mixin and their
greedy reconstructions are drawn on the device (sketchformer_amd/raster.py), every reconstruction into its original's frame,
at 64 x 64 pixels and line width 1.5; the metric is the mean soft IoU (sum min / sum max of the two coverage images).  The
reference has no such metric: it judges reconstructions by eye (metrics/samples.py)."""
import numpy as np

from ..core.metrics import HistoryMetric


class ReconstructionRasterIoU(HistoryMetric):
    name = 'recon-raster-iou'
    input_type = 'predictions_on_validation_set'

    SIZE, LINE_WIDTH = (64, 64), 1.5

    def compute(self, input_data):
        from .. import raster
        x, y, pred_x, pred_y, pred_z, tokenizer, plot_filepath, tmp_filepath, is_continuous = input_data
        x, pred_x = np.asarray(x), np.asarray(pred_x)
        n = min(len(x), len(pred_x))
        if n < 1:
            raise ValueError("recon-raster-iou needs reconstructions (do_reconstruction)")
        if is_continuous:
            orig, recon, kw = x[:n], pred_x[:n, 1:], dict(kind='stroke5')       # row 0 of a reconstruction = start symbol
        else:
            orig, recon, kw = x[:n], pred_x[:n], dict(kind='tokens', tokenizer=tokenizer)
        _, _, iou = raster.render_pair_iou(orig, recon, size=self.SIZE, line_width=self.LINE_WIDTH, **kw)
        return float(iou.double().mean().cpu())
