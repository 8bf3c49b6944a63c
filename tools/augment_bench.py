#!/usr/bin/env python
"""What does the training augmentation cost the continuous train split?  One synthetic chunk of --sketches integer stroke-3
sketches (tools/preprocess_bench.py's: lengths drawn like sketchformer_amd/synthetic.py's, offsets in +-40, a pen lift on ~10 % of
the points and on the last one), the loaders' default hparams with use_continuous_data (augment_stroke_prob 0.1, random_scale_factor
0.1, max_seq_len 200), `preprocess(data, augment=True)` under one numpy seed, and four timings:

  host      DistributedStroke3DataLoader.preprocess - the per-sketch `_augment_sketch` loop, then the numpy block path; wall clock
  previous  what `stroke3-distributed-device` did before the augmentation moved: the same per-sketch host loop, then
            preprocess.encode_chunk(clamp=False) - restated here, with the loader's own `_augment_sketch`; wall clock
  device    the `stroke3-distributed-device` loader's preprocess end to end - packing, the draws, H2D, kernels, D2H; wall clock
  kernels   skf_sketch_augment and skf_sketch_encode (stroke-5) alone on data that is already on the device, HIP events

--repeats timed runs after a warm-up run, the median, and sketches per second.  The three results are compared on the whole chunk.
Set beside what one training rank consumes, batch / --step-ms: pass the ms per step of a continuous bench.py run on the same box, or
leave it out and the README's cfg-3 figure is used and named as such.  Out goes ONE JSON line; with --record also a text record
(profiles/augment_bench.txt).  There is no threshold: the numbers are the finding.

    python tools/augment_bench.py --record profiles/augment_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

README_CFG3_STEP_MS = 15.8          # README.md, cfg 3 (continuous, batch 128): the step time its table quotes


def loader(name):
    """A loader object without chunk files or threads: hparams and clamp limit only."""
    from sketchformer_amd import dataloaders
    cls = dataloaders.get_dataloader_by_name(name)
    hps = cls.default_hparams()
    hps.set_hparam("use_continuous_data", True)
    obj = cls.__new__(cls)
    obj.hps, obj.limit, obj._device = dict(hps.values()), 1000, None
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=70000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-warmup", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--step-ms", type=float, default=None, help="ms per training step of a continuous bench.py run on this box")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from preprocess_bench import make_chunk
    from sketchformer_amd import ops, preprocess
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    data = make_chunk(np, args.sketches, args.seed)
    n_points = int(sum(len(s) for s in data))
    host, device = loader("stroke3-distributed"), loader("stroke3-distributed-device")
    hps = host.hps

    def previous(chunk):
        aug = [host._augment_sketch(np.array(np.clip(s, -1000, 1000), dtype=np.float32)) for s in chunk]
        return preprocess.encode_chunk(aug, hps, None, clamp=False)

    def timed(fn, warm_chunk):
        fn(warm_chunk)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            np.random.seed(args.seed + 7)                   # every leg and every repeat augments under the same draws
            t0 = time.perf_counter()
            out = fn(data)
            ts.append(time.perf_counter() - t0)
        return out, ts

    def leg(ts):
        med = statistics.median(ts)
        return {"s": round(med, 4), "s_all": [round(t, 4) for t in ts], "sketches_per_s": round(args.sketches / med, 1)}

    out = {"tool": "augment_bench", "device": torch.cuda.get_device_name(0), "sketches": args.sketches, "points": n_points,
           "repeats": args.repeats, "max_seq_len": hps["max_seq_len"], "augment_stroke_prob": hps["augment_stroke_prob"],
           "random_scale_factor": hps["random_scale_factor"], "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}
    got, ts = timed(lambda c: device.preprocess(c, augment=True), data)
    out["device_end_to_end"] = leg(ts)
    print("device end to end %s" % out["device_end_to_end"], file=sys.stderr, flush=True)
    prev, ts = timed(previous, data)
    out["previous_device_end_to_end"] = leg(ts)
    print("previous device loader %s" % out["previous_device_end_to_end"], file=sys.stderr, flush=True)
    want, ts = timed(lambda c: host.preprocess(c, augment=True), data[:args.host_warmup])
    out["host"] = leg(ts)
    print("host %s" % out["host"], file=sys.stderr, flush=True)
    out["bit_equal"] = bool(want.dtype == got.dtype and want.shape == got.shape and np.array_equal(want, got))
    out["previous_bit_equal"] = bool(want.dtype == prev.dtype and np.array_equal(want, prev))
    out["speedup_over_host"] = round(out["host"]["s"] / out["device_end_to_end"]["s"], 2)
    out["speedup_over_previous"] = round(out["previous_device_end_to_end"]["s"] / out["device_end_to_end"]["s"], 2)
    # above the spread of the repeats: the slowest new run against the fastest previous one
    out["faster_than_previous_beyond_spread"] = bool(max(out["device_end_to_end"]["s_all"]) < min(out["previous_device_end_to_end"]["s_all"]))
    del want, prev, got

    # the kernels alone: the chunk and the draws packed and uploaded once, events around the launches
    flat, offsets = preprocess.pack_ragged(data)
    np.random.seed(args.seed + 7)
    rnd = np.random.random(size=2 * len(data) + len(flat))
    flat_d, off_d, rnd_d = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(rnd).to(dev)
    e, prob, L = hps["random_scale_factor"], hps["augment_stroke_prob"], hps["max_seq_len"]

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        return {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "sketches_per_s": round(args.sketches / (med * 1e-3), 1)}
    aug_flat, aug_off = ops.sketch_augment(flat_d, off_d, rnd_d, e, prob)
    out["points_kept"] = int(aug_flat.shape[0])
    # (ops.sketch_augment ends in the read of P', which waits for the launches: the events enclose it)
    out["kernels_augment"] = events(lambda: ops.sketch_augment(flat_d, off_d, rnd_d, e, prob))
    out["kernels_encode"] = events(lambda: ops.sketch_encode(aug_flat, aug_off, "stroke5", L, clamp=False))
    if args.step_ms:
        out["step_ms"], out["step_ms_source"] = args.step_ms, "bench.py on this box"
    else:
        out["step_ms"], out["step_ms_source"] = README_CFG3_STEP_MS, "README.md, cfg 3 (not measured in this job)"
    out["rank_consumes_sketches_per_s"] = round(args.batch / (out["step_ms"] * 1e-3), 1)
    print(json.dumps(out))
    if args.record:
        d, p, h = out["device_end_to_end"], out["previous_device_end_to_end"], out["host"]
        with open(args.record, "w") as f:
            f.write("tools/augment_bench.py on %s, %d CPUs: one continuous chunk of %d integer sketches = %d points (%d kept), max_seq_len %d,\n"
                    % (out["device"], out["cpus"], args.sketches, n_points, out["points_kept"], L))
            f.write("augment_stroke_prob %g, random_scale_factor %g, preprocess(augment=True) under one numpy seed; %d timed runs after a warm-up, medians,\n"
                    % (prob, e, args.repeats))
            f.write("all legs in one job on one box.\n\n")
            f.write("sketches per second, one chunk                                          median        every run (s)\n")
            f.write("  one training rank consumes (%d / %.3f ms; %s)   %12.0f\n"
                    % (args.batch, out["step_ms"], out["step_ms_source"], out["rank_consumes_sketches_per_s"]))
            f.write("  host, stroke3-distributed preprocess(augment=True)                %12.0f  (%.4f s)  %s\n" % (h["sketches_per_s"], h["s"], h["s_all"]))
            f.write("  previous stroke3-distributed-device (host loop + encode)          %12.0f  (%.4f s)  %s\n" % (p["sketches_per_s"], p["s"], p["s_all"]))
            f.write("  this stroke3-distributed-device (augment + encode on the device)  %12.0f  (%.4f s)  %s\n" % (d["sketches_per_s"], d["s"], d["s_all"]))
            f.write("  skf_sketch_augment alone, HIP events (incl. the read of P')       %12.0f  (%.4f ms) %s\n"
                    % (out["kernels_augment"]["sketches_per_s"], out["kernels_augment"]["ms"], out["kernels_augment"]["ms_all"]))
            f.write("  skf_sketch_encode (stroke-5) alone, HIP events                    %12.0f  (%.4f ms) %s\n"
                    % (out["kernels_encode"]["sketches_per_s"], out["kernels_encode"]["ms"], out["kernels_encode"]["ms_all"]))
            f.write("\nwhole chunk bit-equal to the host: this loader %s, the previous loader %s\n" % (out["bit_equal"], out["previous_bit_equal"]))
            f.write("this loader over the previous one: %.2f x by the medians; its slowest run %s the previous loader's fastest run\n"
                    % (out["speedup_over_previous"], "beats" if out["faster_than_previous_beyond_spread"] else "DOES NOT beat"))
            f.write("Not measured: how the rest of the end-to-end time splits - packing 70 000 small arrays, the draws (8 bytes a point) and\n"
                    "the input through pageable memory, the (N, L, 5) result back and its cast to float64.\n\n")
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
