"""``stroke3-distributed-device``: ``stroke3-distributed`` with the chunk preprocessing on the device (sketchformer_amd/preprocess.py,
skf_sketch_augment, skf_sketch_encode).  Same hparams, same files, same megabatches - host arrays, bit-equal to the parent's - so the
rest of the loader contract is untouched; only `preprocess` differs."""
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
        # the training augmentation (continuous data) runs on the device as well and consumes the random stream exactly like the
        # parent: two draws per sketch, then one per point (encode_chunk draws them in one call)
        return pre.encode_chunk(data, self.hps, tokenizer, clamp=True, device=self._device, augment=augment)
