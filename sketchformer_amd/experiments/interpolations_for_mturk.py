"""interpolations-for-mturk (experiments/interpolations_for_mturk.py of the reference): for every source sketch one strip of
n_inter sketches on the way to a sketch of its own class (intra) and one on the way to a sketch of another class (inter),
decoded from the slerp of the two embeddings.  The reference gathers the embeddings on the host, interpolates in numpy and
pushes the rows back through predict_from_embedding; here model.interpolate keeps them on the device from the encoder to the
decoder.  The reference draws the strips with svgwrite (utils/skt_tools.py: make_grid_svg, draw_strokes3); this one writes the
SVG text itself."""
import os

import numpy as np

from ..core.experiments import Experiment
from ..metrics.samples import stroke5_to_stroke3, strokes_to_lines
from ..utils import hparams as hp


def write_strip_svg(sketches, path, cell=100.0, margin=5.0):
    """One row of stroke-3 sketches, one <path> of M / L commands each.  A sketch is scaled into its cell by the larger side of
    its bounds; an empty sketch, a single point or non-finite offsets still give one path with finite coordinates."""
    n = len(sketches)
    parts = ['<?xml version="1.0" encoding="utf-8"?>',
             '<svg xmlns="http://www.w3.org/2000/svg" version="1.1" width="%g" height="%g" viewBox="0 0 %g %g">'
             % (cell * max(n, 1), cell, cell * max(n, 1), cell),
             '<rect x="0" y="0" width="%g" height="%g" fill="white"/>' % (cell * max(n, 1), cell)]
    inner = cell - 2 * margin
    for k, sketch in enumerate(sketches):
        s = np.nan_to_num(np.asarray(sketch, dtype=np.float64).reshape(-1, 3), posinf=0.0, neginf=0.0)
        lines = strokes_to_lines(s) if len(s) else []
        cmds = []
        if lines:
            pts = np.concatenate(lines, axis=0)
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            side = float(max(hi[0] - lo[0], hi[1] - lo[1]))
            if not np.isfinite(side) or side <= 0.0:
                side = 1.0
            off = np.array([k * cell + margin, margin]) + (inner - (hi - lo) / side * inner) / 2.0   # centred in the cell
            for ln in lines:
                xy = (ln - lo) / side * inner + off
                cmds.append("M %.3f %.3f" % (xy[0, 0], xy[0, 1]))
                cmds.extend("L %.3f %.3f" % (x, y) for x, y in xy[1:])
        else:
            cmds.append("M %.3f %.3f" % (k * cell + cell / 2.0, cell / 2.0))
        parts.append('<path d="%s" fill="none" stroke="black" stroke-width="1" stroke-linecap="round"/>' % " ".join(cmds))
    parts.append('</svg>')
    with open(path, "w") as f:
        f.write("\n".join(parts) + "\n")
    return path


class InterpolationsForMturk(Experiment):
    name = "interpolations-for-mturk"
    requires_model = True

    @classmethod
    def specific_default_hparams(cls):
        # the reference's defaults are paths of its authors' cluster; n_inter is hard-coded to 10 there (:101)
        return hp.HParams(source_emb='', intra_emb='', inter_emb='', batch_size=256, n_inter=10, mode='slerp')

    def _load(self, key):
        path = self.hps[key]
        if not path or not os.path.isfile(path):
            raise ValueError("interpolations-for-mturk: hparam %s=%r is not a file; it must name an .npz with 'data' (stroke-3 "
                             "sketches), 'cat' and 'ids'" % (key, path))
        return np.load(path, allow_pickle=True)

    @staticmethod
    def _to_sketches(model, recon):
        if model.dataset.hps['use_continuous_data']:
            return [stroke5_to_stroke3(r[1:]) for r in recon]              # row 0 of a reconstruction = start symbol
        return model.dataset.tokenizer.decode(list(recon))

    def compute(self, model=None):
        files = {'src': self._load('source_emb'), 'intra': self._load('intra_emb'), 'inter': self._load('inter_emb')}
        y_data = {k: f['cat'] for k, f in files.items()}
        id_data = {k: f['ids'] for k, f in files.items()}
        # the reference's np.squeeze (:44) drops the token column of (N, L, 1); only that axis here, so one sketch stays a batch
        squeeze = (lambda x: x) if model.dataset.hps['use_continuous_data'] else (lambda x: np.squeeze(x, axis=-1))
        x_data = {k: squeeze(model.dataset.preprocess_extra_sets_from_interp_experiment(f['data'])) for k, f in files.items()}
        n_src = len(x_data['src'])
        for k in ('intra', 'inter'):
            if len(x_data[k]) != n_src:
                raise ValueError("interpolations-for-mturk: %s_emb holds %d sketches, source_emb %d" % (k, len(x_data[k]), n_src))
        bs = min(self.hps['batch_size'], model.hps['batch_size'])          # the engine's batch is its capacity per call
        obj = lambda lst: np.array(list(lst) + [None], dtype=object)[:-1]    # ragged lists -> object arrays  # noqa: E731

        interp_dir = os.path.join(self.out_dir, 'interpolations')
        recon_dir = os.path.join(self.out_dir, 'reconstructions')
        for d in (interp_dir, os.path.join(interp_dir, 'intra'), os.path.join(interp_dir, 'inter'), recon_dir):
            os.makedirs(d, exist_ok=True)

        # reconstruction of the sources (:62-96)
        src_recon = []
        for i in range(0, n_src, bs):
            z = model.predict_class(x_data['src'][i:i + bs])['embedding']
            src_recon.extend(list(model.predict_from_embedding(z, expected_len=None)['recon']))
        np.savez(os.path.join(recon_dir, 'reconstructed_source.npz'), recon=obj(self._to_sketches(model, src_recon)),
                 cat=y_data['src'], ids=id_data['src'])

        n_inter = int(self.hps['n_inter'])
        for set_type in ('intra', 'inter'):
            res = model.interpolate(x_data['src'], x_data[set_type], n_inter, self.hps['mode'])
            recon = res['recon']
            names = []
            for i in range(n_src):
                name = "{:03d}_slerp_{}_{}_{}_{}.svg".format(i, y_data['src'][i], y_data[set_type][i], id_data['src'][i],
                                                             id_data[set_type][i])
                strip = [np.nan_to_num(s) for s in self._to_sketches(model, recon[i])]
                write_strip_svg(strip, os.path.join(interp_dir, set_type, name))
                names.append(name)
            np.savez(os.path.join(interp_dir, set_type + '.npz'), embedding=res['embedding'], recon=recon,
                     cat_src=y_data['src'], cat_dst=y_data[set_type], ids_src=id_data['src'], ids_dst=id_data[set_type],
                     files=np.array(names))
        return interp_dir
