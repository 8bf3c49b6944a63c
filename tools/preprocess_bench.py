#!/usr/bin/env python
"""Does chunk preprocessing feed the training step?  One synthetic chunk of --sketches integer stroke-3 sketches (lengths drawn like
sketchformer_amd/synthetic.py's, offsets in +-40, a pen lift on ~10 % of the points and on the last one), two tokenizers - a
K = 1000 `.npz` dictionary and the 100 x 100 grid - and per tokenizer three timings:

  host    DistributedStroke3DataLoader.preprocess (the numpy block path), wall clock
  device  the `stroke3-distributed-device` loader's preprocess end to end - packing, H2D, kernels, D2H - wall clock
  kernels skf_sketch_encode alone on data that is already on the device, HIP events

--repeats timed runs after a warm-up run, the median, and sketches per second.  Set beside what one training rank consumes,
batch / (ms per step of bench.py's head on the same box): pass that figure with --step-ms.  The host dictionary leg is a chunked
float64 argmin over 1000 centres and takes tens of seconds per run; its warm-up run uses the first --host-warmup sketches only.
There is no threshold: the numbers are the finding.  Out goes ONE JSON line.

    python tools/preprocess_bench.py --step-ms 3.45
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_chunk(np, n, seed):
    from sketchformer_amd import synthetic
    rng = np.random.RandomState(seed)
    lens = synthetic._lengths(rng, n, 200)
    data = np.empty(n, dtype=object)
    for i in range(n):
        m = int(lens[i])
        s = np.zeros((m, 3), dtype=np.int16)
        s[:, :2] = rng.randint(-40, 41, size=(m, 2))
        s[:, 2] = rng.rand(m) < 0.1
        s[-1, 2] = 1
        data[i] = s
    return data


def loader(name, tokenizer, token_type):
    """A loader object without chunk files or threads: hparams, clamp limit and tokenizer only."""
    from sketchformer_amd import dataloaders
    cls = dataloaders.get_dataloader_by_name(name)
    hps = cls.default_hparams()
    hps.set_hparam("token_type", token_type)
    obj = cls.__new__(cls)
    obj.hps, obj.limit, obj.tokenizer, obj._device = dict(hps.values()), 1000, tokenizer, None
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=70000)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-warmup", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--step-ms", type=float, default=None, help="ms per training step of bench.py's head on this box")
    ap.add_argument("--no-host", action="store_true", help="skip the host legs")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from sketchformer_amd import ops, preprocess
    from sketchformer_amd.utils.tokenizer import GridTokenizer, Tokenizer
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    data = make_chunk(np, args.sketches, args.seed)
    n_points = int(sum(len(s) for s in data))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "dict.npz")
        centers = np.random.RandomState(args.seed + 1).uniform(-0.6, 0.6, size=(args.K, 2)).astype(np.float32)
        np.savez(path, cluster_centers=centers, inertia=np.float64(0), n_iter=np.int64(1))
        tokenizers = {"dictionary": Tokenizer(path, max_seq_len=0), "grid": GridTokenizer(resolution=100)}

    def timed(fn, warm):
        warm()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return out, ts

    def leg(ts):
        med = statistics.median(ts)
        return {"s": round(med, 4), "s_all": [round(t, 4) for t in ts], "sketches_per_s": round(args.sketches / med, 1)}

    out = {"tool": "preprocess_bench", "sketches": args.sketches, "points": n_points, "K": args.K, "repeats": args.repeats,
           "max_seq_len": 200, "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    for name, tok in tokenizers.items():
        rec = {}
        host, device = loader("stroke3-distributed", tok, name), loader("stroke3-distributed-device", tok, name)
        got, ts = timed(lambda: device.preprocess(data), lambda: device.preprocess(data))
        rec["device_end_to_end"] = leg(ts)
        print("%s: device end to end %s" % (name, rec["device_end_to_end"]), file=sys.stderr, flush=True)
        if not args.no_host:
            want, ts = timed(lambda: host.preprocess(data), lambda: host.preprocess(data[:args.host_warmup]))
            rec["host"] = leg(ts)
            print("%s: host %s" % (name, rec["host"]), file=sys.stderr, flush=True)
            rec["bit_equal"] = bool(want.dtype == got.dtype and np.array_equal(want, got))
            rec["speedup_end_to_end"] = round(rec["host"]["s"] / rec["device_end_to_end"]["s"], 2)
        # the kernels alone: the chunk packed and uploaded once, events around the launches
        flat, offsets = preprocess.pack_ragged(data)
        flat_d, off_d = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
        kw = {"centers": torch.from_numpy(tok.centers).to(dev)} if name == "dictionary" else {"resolution": tok.resolution}
        mode = "dict" if name == "dictionary" else "grid"
        ops.sketch_encode(flat_d, off_d, mode, 200, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); ops.sketch_encode(flat_d, off_d, mode, 200, **kw); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        rec["kernels"] = {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "sketches_per_s": round(args.sketches / (med * 1e-3), 1)}
        if name == "dictionary":
            rec["kernels"]["pairs_per_s"] = round(float(n_points) * args.K / (med * 1e-3), 1)
        out[name] = rec
    if args.step_ms:
        out["step_ms"] = args.step_ms
        out["rank_consumes_sketches_per_s"] = round(args.batch / (args.step_ms * 1e-3), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
