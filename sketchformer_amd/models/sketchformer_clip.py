"""``sketch-transformer-tf2-clip``: the sketch transformer with gradient clipping, a gradient-norm read-out and a guard
against non-finite gradients (TrainEngine.set_gradient_clip).  The hparams of ``sketch-transformer-tf2`` are the reference's and
stay as they are; this model adds its own on top, shares variables and checkpoints with the parent, and is found by the registry
like every subclass of BaseModel.
"""
import json
import os

from ..utils.hparams import HParams, combine_hparams_into_one
from .sketchformer import Transformer


class ClippedTransformer(Transformer):
    name = 'sketch-transformer-tf2-clip'
    quick_metrics = Transformer.quick_metrics + ['grad_norm', 'skipped_steps']

    @classmethod
    def clip_default_hparams(cls):
        """clipnorm / global_clipnorm / clipvalue: tf.keras optimizers' arguments, 0 = off, at most one of them; skip_nonfinite:
        a step with an inf / NaN gradient changes nothing and is counted; grad_report_every: every that many steps one JSON line
        of per-variable gradient and weight norms goes to grad_norms.jsonl in the model's output directory (0 = never)."""
        return HParams(clipnorm=0.0, global_clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False, grad_report_every=0)

    @classmethod
    def specific_default_hparams(cls):
        return combine_hparams_into_one(Transformer.specific_default_hparams(), cls.clip_default_hparams())

    def build_model(self):
        from .. import engine
        h = self.hps
        engine.check_gradient_clip(h['clipnorm'], h['global_clipnorm'], h['clipvalue'])      # before anything is allocated
        if h['grad_report_every'] < 0:
            raise ValueError("grad_report_every must be >= 0")
        super().build_model()
        # monitor: the quick metric grad_norm needs the norms whatever else is configured
        self.engine.set_gradient_clip(clipnorm=h['clipnorm'], global_clipnorm=h['global_clipnorm'], clipvalue=h['clipvalue'],
                                      skip_nonfinite=h['skip_nonfinite'], monitor=True)
        self.grad_report_path = os.path.join(self.out_dir, 'grad_norms.jsonl')
        self._steps_taken = 0

    def train_on_batch(self, batch):
        res = super().train_on_batch(batch)       # (its snapshot carries the statistics words: no read-back here)
        self._steps_taken += 1
        every = self.hps['grad_report_every']
        if every and self._steps_taken % every == 0:
            self.write_grad_report()
        return res

    def write_grad_report(self):
        """One JSON line: step, global norm, scale, skipped total, per-variable gradient and weight norms (one extra read-back)."""
        rep = self.engine.gradient_report()
        if self.rank != 0:
            return
        line = {'step': int(self.engine.iterations), 'grad_norm': rep['global_norm'], 'scale': rep['scale'],
                'skipped_steps': rep['skipped_total'], 'weight_norm': rep['weight_global_norm'],
                'grad_norms': {k: v['grad_norm'] for k, v in rep['variables'].items()},
                'weight_norms': {k: v['weight_norm'] for k, v in rep['variables'].items()}}
        with open(self.grad_report_path, 'a') as f:
            f.write(json.dumps(line) + "\n")
