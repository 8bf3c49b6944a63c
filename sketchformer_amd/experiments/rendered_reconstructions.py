"""rendered-reconstructions: seeded sketches of a split and their greedy reconstructions as images, with a score.  The model
reconstructs (model.predict), the device rasterizer (sketchformer_amd/raster.py) draws every reconstruction into its original's
frame and the soft IoU of the two coverage images says how much of the drawing came back.  Writes one .npz (originals and
reconstructions as uint8 images, the sketches they were drawn from, iou per sketch, mean_iou) and one PNG contact sheet, original
and reconstruction interlaced, 6 per row - the layout of the reference's build_interlaced_grid_list (utils/sketch.py)."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..utils import hparams as hp


class RenderedReconstructions(Experiment):
    name = "rendered-reconstructions"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        return hp.HParams(n_sketches=32, split='valid', size=128, line_width=1.5,
                          target_file='rendered_reconstructions.npz', plot_file='rendered_reconstructions.png')

    def _path(self, key):
        p = self.hps[key]
        return p if os.path.isabs(p) else os.path.join(self.out_dir, p)

    def compute(self, model=None):
        from .. import raster
        h = self.hps
        n, size = int(h['n_sketches']), int(h['size'])
        if n < 1:
            raise ValueError("rendered-reconstructions: n_sketches must be >= 1")
        continuous = bool(model.dataset.hps['use_continuous_data'])
        x, _ = model.dataset.get_n_samples_from(h['split'], n, shuffled=True, seeded=True)
        x = np.asarray(x)[:n]
        if not continuous and x.ndim == 3:
            x = np.squeeze(x, axis=-1)                                   # (N, L, 1) token columns of the file loaders
        n = len(x)
        bs = model.hps['batch_size']                                     # the engine's batch is its capacity per call
        recon = None
        for i in range(0, n, bs):
            r = np.asarray(model.predict(x[i:i + bs])['recon'])
            if recon is None:
                recon = np.zeros((n, model.seq_len + 1) + r.shape[2:], dtype=r.dtype)     # batches stop at different lengths
            recon[i:i + len(r), :r.shape[1]] = r
        if continuous:
            drawn, kw = recon[:, 1:], dict(kind='stroke5')               # row 0 of a reconstruction = start symbol
        else:
            drawn, kw = recon, dict(kind='tokens', tokenizer=model.dataset.tokenizer)
        a, b, iou = raster.render_pair_iou(x, drawn, size=(size, size), line_width=float(h['line_width']), **kw)
        a8, b8 = raster.to_uint8(a), raster.to_uint8(b)
        iou = iou.cpu().numpy()
        plot = raster.save_png(self._path('plot_file'), raster.contact_sheet(raster.interlace(a8, b8), cols=6, pad=2))
        target = self._path('target_file')
        np.savez(target, originals=a8, reconstructions=b8, iou=iou, mean_iou=np.float64(iou.astype(np.float64).mean()),
                 inputs=x, recon=recon, size=np.int32(size), line_width=np.float32(h['line_width']),
                 plot=np.array(os.path.basename(plot)))
        return target
