"""``sketch-transformer-tf2-accum``: the clipped sketch transformer with gradient accumulation - ``accum_steps`` micro-batches of
``batch_size`` rows per optimizer step (TrainEngine.set_gradient_accumulation), so the effective batch is
batch_size * accum_steps * world_size while the activation workspace stays that of one micro-batch, and under data parallelism the
gradient all-reduce runs once per optimizer step.  It subclasses the clip model - clipping, the norms and the non-finite guard act on
the accumulated (mean) gradient - shares variables and checkpoints with its parents, and is found by the registry like every subclass
of BaseModel.  The parents and their hparams are untouched.
"""
from ..utils.hparams import HParams, combine_hparams_into_one
from .sketchformer_clip import ClippedTransformer


class AccumulatedTransformer(ClippedTransformer):
    name = 'sketch-transformer-tf2-accum'

    @classmethod
    def accum_default_hparams(cls):
        """accum_steps: micro-batches per optimizer step, 1 = none.  ``batch_size`` stays the size of a micro-batch; the loop's
        step counter (log_every, checkpoints, batches per epoch) counts micro-batches, ``engine.iterations``, the learning-rate
        schedule, ``skipped_steps`` and ``grad_report_every`` count optimizer steps."""
        return HParams(accum_steps=1)

    @classmethod
    def specific_default_hparams(cls):
        return combine_hparams_into_one(ClippedTransformer.specific_default_hparams(), cls.accum_default_hparams())

    def build_model(self):
        from .. import engine
        engine.check_gradient_accumulation(self.hps['accum_steps'])      # before anything is allocated
        super().build_model()
        self.engine.set_gradient_accumulation(self.hps['accum_steps'])

    def train_on_batch(self, batch):
        """One micro-batch.  On a micro-step that does not close an optimizer step nothing is applied: ``grad_norm`` and
        ``skipped_steps`` in the result are those of the last applied step, and no gradient report is due."""
        before = self.engine.accumulation_pending
        res = super(ClippedTransformer, self).train_on_batch(batch)       # Transformer's: the clip model's counts every call
        if self.engine.accumulation_pending > before:
            return res                                                    # still open
        self._steps_taken += 1
        every = self.hps['grad_report_every']
        if every and self._steps_taken % every == 0:
            self.write_grad_report()
        return res

    def load_state_dict(self, state):
        """Checkpoints do not carry pending micro-batches: a restored model starts a new optimizer step (what was summed before the
        save, if anything, is discarded on restore - save on a multiple of accum_steps to lose nothing)."""
        self.engine.reset_accumulation()
        super().load_state_dict(state)
