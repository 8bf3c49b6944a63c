"""Chunk preprocessing on the device: raw stroke-3 sketches -> model input through skf_sketch_encode (include/skf.h, DESIGN.md
section 3m).  The host code of dataloaders/distributed_stroke3.py stays the definition; what comes back from here is bit-equal to
its `preprocess` - same values, same dtype, same shape.

A pickled sklearn dictionary is used through its `cluster_centers_` cast to float64: the device rule is the numpy rule of
Tokenizer.nearest_center (float64 distances, first minimum wins); sklearn's own `predict` computes in the dtype of the fitted
centres through an expanded form of the distance and may differ from it on exact near-ties.
"""
import numpy as np

from .utils.tokenizer import GridTokenizer, Tokenizer


def pack_ragged(data):
    """Object array / list of stroke-3 arrays -> (flat float32 (P, 3), offsets int64 (N + 1)): the sketches back to back, sketch i
    in rows offsets[i] .. offsets[i + 1] - 1.  Columns behind the third are dropped, like the loader does."""
    n = len(data)
    lens = np.fromiter((len(s) for s in data), dtype=np.int64, count=n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    parts = [np.asarray(s)[:, :3] for s in data if len(s)]
    flat = np.concatenate(parts, axis=0).astype(np.float32, copy=False) if parts else np.zeros((0, 3), dtype=np.float32)
    return np.ascontiguousarray(flat), offsets


def _device(device):
    """The device a call runs on: the current one unless the caller names one."""
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def device_path_supported(hps, tokenizer):
    """The conditions on the hparams / tokenizer under which DistributedStroke3DataLoader.preprocess takes its block path (and the
    device loader the device): no stroke shuffling, offsets not absolute, and continuous data or one of the two tokenizers."""
    return bool(not hps["shuffle_stroke"] and not hps["use_absolute_strokes"]
                and (hps["use_continuous_data"] or isinstance(tokenizer, (GridTokenizer, Tokenizer))))


def encode_chunk(data, hps, tokenizer, clamp=True, device=None, stream=None, augment=False):
    """One chunk of stroke-3 sketches -> what `preprocess` returns for it: int64 (N, L) tokens, or float64 (N, L, 5) stroke-5 rows
    (cast up from the device's float32, which is exact).  clamp: clamp every column to +-1000 first (off for sketches that were
    clamped before an augmentation).  augment: the training augmentation, on the device too (ops.sketch_augment, DESIGN.md section
    3o) and exactly where the host applies it - continuous data with augment_stroke_prob > 0; it consumes the global numpy stream
    like the host, 2 N + P draws in one call, and nothing in token modes or at augment_stroke_prob == 0.  Runs on a side stream of
    its own - the loader calls this from its background thread while the training thread issues steps - and synchronises only
    that stream."""
    if not device_path_supported(hps, tokenizer):
        raise ValueError("these hparams have no device path (device_path_supported)")
    if len(data) == 0:
        raise ValueError("encode_chunk needs at least one sketch")
    if min(len(s) for s in data) == 0:
        raise IndexError("empty sketch")                      # like preprocess_per_sketch_from, before the device is touched
    flat, offsets = pack_ragged(data)
    if offsets[0] != 0 or offsets[-1] != len(flat) or (np.diff(offsets) < 0).any():      # the kernels only clamp what they read
        raise ValueError("offsets must run from 0 to the number of points without decreasing")
    import torch
    from . import ops
    dev = _device(device)
    side = torch.cuda.Stream(device=dev) if stream is None else stream
    L = int(hps["max_seq_len"])
    with torch.cuda.device(dev), torch.cuda.stream(side):
        flat_d = torch.from_numpy(flat).to(dev)
        off_d = torch.from_numpy(offsets).to(dev)
        if augment and hps["use_continuous_data"] and hps["augment_stroke_prob"] > 0:
            # the host's draws in the host's order (two per sketch, then one per point), replayed by the device; the clamp comes
            # before the augmentation, like the reference, and not again behind it
            rnd_d = torch.from_numpy(np.random.random(size=2 * len(data) + len(flat))).to(dev)
            flat_d, off_d = ops.sketch_augment(flat_d, off_d, rnd_d, hps["random_scale_factor"], hps["augment_stroke_prob"], clamp=clamp)
            out = ops.sketch_encode(flat_d, off_d, 'stroke5', L, clamp=False)
        elif hps["use_continuous_data"]:
            out = ops.sketch_encode(flat_d, off_d, 'stroke5', L, clamp=clamp)
        elif isinstance(tokenizer, GridTokenizer):
            out = ops.sketch_encode(flat_d, off_d, 'grid', L, resolution=tokenizer.resolution, clamp=clamp)
        else:
            centers = torch.from_numpy(np.ascontiguousarray(tokenizer.centers, dtype=np.float64)).to(dev)
            out = ops.sketch_encode(flat_d, off_d, 'dict', L, centers=centers, clamp=clamp)
        host = out.cpu()                                      # a blocking copy on the side stream
        side.synchronize()
    res = host.numpy()
    return res.astype(np.float64) if hps["use_continuous_data"] else res
