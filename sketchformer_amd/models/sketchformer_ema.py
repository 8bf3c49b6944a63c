"""``sketch-transformer-tf2-ema``: the accumulating, clipped sketch transformer with weight averaging - an exponential moving average
of the weights (tf.train.ExponentialMovingAverage / tfa.optimizers.MovingAverage; TrainEngine.set_weight_average) that evaluation
and sampling run on.  Every optimizer step ends with one more launch over the flat parameter buffer; the average lives in a shadow
buffer of the same size.  With ``ema_eval`` every public inference entry of ``Transformer`` runs on the averaged weights: the first
inference call after training swaps the shadow into ``params`` (one launch), the next ``train_on_batch`` / ``state_dict`` /
``_save`` / ``load_state_dict`` swaps back - alternating evaluation and training costs two swap launches per transition and nothing
per call.  It subclasses the accumulation model, shares variables with its parents, and is found by the registry like every
subclass of BaseModel.  The parents and their hparams are untouched.

Checkpoints: ``state_dict`` is taken with the raw weights in ``params`` and gains the key ``'ema'``, the shadow.  The parents load
such a checkpoint unchanged (they ignore the key).  A checkpoint WITHOUT the key - one a parent model wrote - loads with
shadow = params: the average starts over from the restored weights, as a fresh tf shadow variable does.
"""
import functools

from ..utils.hparams import HParams, combine_hparams_into_one
from .sketchformer_accum import AccumulatedTransformer

# every public inference entry of Transformer (models/sketchformer.py) and the slow-metrics paths of BaseModel that drive them
AVERAGED_ENTRIES = ('encode_from_seq', 'predict_class', 'predict_from_embedding', 'predict', 'beam_search_from_embedding', 'beam_search',
                    'interpolate', 'sample_from_embedding', 'sample', 'complete_from_embedding', 'complete', 'score',
                    'compute_metrics_from', 'compute_all_metrics')


def _on_average(name):
    inner = getattr(AccumulatedTransformer, name)

    @functools.wraps(inner)
    def entry(self, *args, **kw):
        self._swap_in_average()
        return inner(self, *args, **kw)
    return entry


class AveragedTransformer(AccumulatedTransformer):
    name = 'sketch-transformer-tf2-ema'

    @classmethod
    def ema_default_hparams(cls):
        """ema_decay: the decay of the average, in (0, 1); 0 = no averaging (the parent model, launch for launch).  ema_num_updates:
        the warm-up rule min(decay, (1 + n) / (10 + n)) over n = optimizer steps applied, so that an early average is not dominated by
        the initial weights.  ema_eval: inference and the slow metrics run on the averaged weights (False: the average is kept and
        saved, but nothing reads it - ``engine.averaged_weights()`` does by hand)."""
        return HParams(ema_decay=0.0, ema_num_updates=True, ema_eval=True)

    @classmethod
    def specific_default_hparams(cls):
        return combine_hparams_into_one(AccumulatedTransformer.specific_default_hparams(), cls.ema_default_hparams())

    def build_model(self):
        from .. import engine
        decay = self.hps['ema_decay']
        if decay != 0:
            engine.check_weight_average(decay)      # before anything is allocated
        super().build_model()
        self._lazy_average = bool(decay != 0 and self.hps['ema_eval'])
        if decay != 0:
            self.engine.set_weight_average(decay, num_updates=self.hps['ema_num_updates'])

    # ---- the lazy swap
    def _swap_in_average(self):
        if self._lazy_average and not self.engine.average_live:
            self.engine.swap_weight_average()

    def _swap_out_average(self):
        if self.engine.average_live:
            self.engine.swap_weight_average()

    def train_on_batch(self, batch):
        self._swap_out_average()
        return super().train_on_batch(batch)

    # ---- checkpoints
    def state_dict(self):
        self._swap_out_average()
        state = super().state_dict()
        avg = self.engine.weight_average
        if avg is not None:
            state['ema'] = avg.cpu()
        return state

    def _save(self, path):
        self._swap_out_average()      # on every rank (state_dict runs on rank 0 alone)
        super()._save(path)

    def load_state_dict(self, state):
        """Restores the shadow from ``'ema'``; a checkpoint without the key (a parent model's) loads with shadow = params."""
        self._swap_out_average()
        super().load_state_dict(state)
        e = self.engine
        if e.weight_average is None:
            return
        if 'ema' in state:
            e.weight_average.copy_(state['ema'])
            e.assert_replicas_equal()
        else:
            e.reset_weight_average()

    def load_reference_checkpoint(self, prefix):
        """The reference trains without an average: shadow = the restored weights."""
        self._swap_out_average()
        super().load_reference_checkpoint(prefix)
        if self.engine.weight_average is not None:
            self.engine.reset_weight_average()


for _name in AVERAGED_ENTRIES:
    setattr(AveragedTransformer, _name, _on_average(_name))
del _name
