"""``stroke3-distributed-device``: ``stroke3-distributed`` with the chunk preprocessing on the device (sketchformer_amd/preprocess.py,
skf_sketch_encode).  Same hparams, same files, same megabatches - host arrays, bit-equal to the parent's - so the rest of the
loader contract is untouched; only `preprocess` differs."""
import numpy as np

from .. import preprocess as pre
from .distributed_stroke3 import DistributedStroke3DataLoader


class DeviceStroke3DataLoader(DistributedStroke3DataLoader):
    name = "stroke3-distributed-device"

    def __init__(self, hps, data_directory):
        import torch
        self._device = torch.cuda.current_device()       # the constructing thread's device: chunks are loaded by background threads
        super().__init__(hps, data_directory)

    def preprocess(self, data, augment=False):
        tokenizer = getattr(self, "tokenizer", None)
        if len(data) == 0 or not pre.device_path_supported(self.hps, tokenizer):
            return super().preprocess(data, augment)
        if min(len(s) for s in data) == 0:
            raise IndexError("empty sketch")
        if augment and self.hps["augment_stroke_prob"] > 0 and self.hps["use_continuous_data"]:
            # scale + point dropping stay per sketch on the host and consume the random stream exactly like the parent: two draws,
            # then one per point.  The sketches are clamped before the augmentation, like the reference, so not again behind it
            data = [self._augment_sketch(np.array(np.clip(s, -self.limit, self.limit), dtype=np.float32)) for s in data]
            return pre.encode_chunk(data, self.hps, tokenizer, clamp=False, device=self._device)
        return pre.encode_chunk(data, self.hps, tokenizer, clamp=True, device=self._device)
