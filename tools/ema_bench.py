#!/usr/bin/env python
"""What weight averaging costs a train step, at the cfg-2 (fp32, B = 128) and cfg-5 (bf16, B = 8) dimensions.
    python tools/ema_bench.py [--rounds 6] [--steps 20] [--record profiles/ema_bench.txt] [--parent-tree DIR]
  (a) ms per step of train_step: averaging off, on (decay 0.999 with the num_updates ramp) and on together with a global clip and
      the non-finite guard (the update then reads the skip word).  One engine per config; the variants alternate inside one process
      (off ema ema_clip, repeated `rounds` times), every window is `steps` steps between a device synchronise and the next, after
      two warm-up steps of that variant.
  (b) the update launch alone (shadow -= (shadow - params) * (1 - d): two reads, one write) and a swap alone (two reads, two writes)
      on the config's parameter buffer, and their bytes/s beside a device copy of the same buffer in the same run (in turns).
  --parent-tree DIR   also time the unconfigured step on the package under DIR (a build of the parent commit): child processes, this
                      tree and that one in turns (the two libraries cannot share a process), three rounds each
  --off-only          what such a child runs: the unconfigured step alone, on the package of --tree, one JSON line per config"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--record")
ap.add_argument("--parent-tree")
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch                                     # noqa: E402
from sketchformer_amd import engine, synthetic   # noqa: E402

DECAY = 0.999
CONFIGS = {
    "cfg2": dict(batch=128, kw=dict(seq_len=200, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=1004, n_classes=345, lowerdim=256,
                                    dropout_rate=0.1, seed=1234, act_dtype="f32")),
    "cfg5": dict(batch=8, kw=dict(seq_len=512, d_model=512, num_heads=8, dff=2048, num_layers=8, vocab_size=1004, n_classes=345, lowerdim=256,
                                  dropout_rate=0.1, seed=1234, act_dtype="bf16")),
}
VARIANTS = [("off", None, {}), ("ema", DECAY, {}), ("ema_clip", DECAY, dict(global_clipnorm=1e-3, skip_nonfinite=True))]


def build(name):
    c = CONFIGS[name]
    eng = engine.TrainEngine(engine.make_config(batch=c["batch"], use_graph=False, **c["kw"]), init_seed=0)
    eng.state[0] = 3000                          # lr != 0
    xs, ys = synthetic.token_batch(c["batch"], c["kw"]["seq_len"], c["kw"]["vocab_size"], c["kw"]["n_classes"], seed=0)
    return eng, torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()


def window(eng, x, y, steps, warmup=2):
    for _ in range(warmup):
        eng.train_step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.train_step(x, y)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def stats(ts):
    ts = np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "n": int(len(ts))}


if args.off_only:
    for name in CONFIGS:
        eng, x, y = build(name)
        window(eng, x, y, args.steps, warmup=5)
        print(json.dumps(dict(stats([window(eng, x, y, args.steps) for _ in range(args.rounds)]), config=name)))
        del eng
        torch.cuda.empty_cache()
    sys.exit(0)

from sketchformer_amd import ops                 # noqa: E402


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps      # us per call


lines = ["tools/ema_bench.py on %s: train_step (forward, backward, optimizer, weight-average update) with synthetic batches, dropout 0.1, "
         "eager launches" % torch.cuda.get_device_name(0),
         "ms per step; windows of %d steps between two device synchronises, two warm-up steps of the variant first, variants in turns, "
         "%d rounds; decay %g with the num_updates ramp; ema_clip - off contains the clip's own launches" % (args.steps, args.rounds, DECAY), ""]
result = {}
for name in CONFIGS:
    eng, x, y = build(name)
    window(eng, x, y, args.steps, warmup=5)
    times = {v: [] for v, _, _ in VARIANTS}
    for _ in range(args.rounds):
        for v, decay, clip in VARIANTS:
            eng.set_gradient_clip(**clip)
            eng.set_weight_average(decay, num_updates=True)
            times[v].append(window(eng, x, y, args.steps))
    seen = eng.gradient_stats()
    lag = float((eng.weight_average - eng.params).abs().max())
    eng.set_weight_average(None)
    eng.set_gradient_clip()
    table = {v: stats(ts) for v, ts in times.items()}
    off = table["off"]
    n_par = sum(e["rows"] * e["cols"] for e in eng.entries)
    lines += ["%s: B = %d, %s, %d parameters, flat buffer %d floats (%.1f MB)"
              % (name, CONFIGS[name]["batch"], CONFIGS[name]["kw"]["act_dtype"], n_par, eng.n_floats, 4 * eng.n_floats / 1e6),
              "  %-13s %10s %10s %10s %18s" % ("variant", "median ms", "min ms", "max ms", "median - off")]
    for v, _, _ in VARIANTS:
        s = table[v]
        lines.append("  %-13s %10.3f %10.3f %10.3f %+10.3f ms (%+.2f %%)" % (v, s["median_ms"], s["min_ms"], s["max_ms"], s["median_ms"] - off["median_ms"],
                                                                              100.0 * (s["median_ms"] - off["median_ms"]) / off["median_ms"]))
    lines.append("  spread of the off windows (max - min): %.3f ms; last clipped step: skipped %d of them, scale %.4g; the shadow lags the "
                 "weights by at most %.3g" % (off["max_ms"] - off["min_ms"], seen["skipped_total"], seen["scale"], lag))
    # (b) the update and the swap alone, beside a device copy of the same buffer
    w = eng.params
    shadow, other, dst = w.clone(), w.clone(), torch.empty_like(w)
    st = eng.state
    update = lambda: ops.ema_update(shadow, w, DECAY, True, st)                                          # noqa: E731
    swap = lambda: ops.buffer_swap(shadow, other)                                                        # noqa: E731
    copy = lambda: dst.copy_(w)                                                                          # noqa: E731
    for fn in (update, swap, copy):
        events(fn, 20)
    us = {"update": [], "swap": [], "copy": []}
    for _ in range(args.rounds):
        us["update"].append(events(update, 50))
        us["swap"].append(events(swap, 50))
        us["copy"].append(events(copy, 50))
    nb = 4 * w.numel()
    mu, ms, mc = (float(np.median(us[n])) for n in ("update", "swap", "copy"))
    rate = lambda passes, t: passes * nb / (t * 1e-6) / 1e9                                              # noqa: E731
    lines += ["  update launch alone (50 back-to-back calls per window): %.1f us per call, %.2f MB read twice + written once -> %.0f GB/s "
              "= %.0f %% of the copy's byte rate" % (mu, nb / 1e6, rate(3, mu), 100.0 * rate(3, mu) / rate(2, mc)),
              "  swap launch alone: %.1f us per call, %.2f MB read twice + written twice -> %.0f GB/s = %.0f %% of the copy's byte rate"
              % (ms, nb / 1e6, rate(4, ms), 100.0 * rate(4, ms) / rate(2, mc)),
              "  device copy of the flat buffer in the same run: %.1f us per call, %.2f MB read + as much written -> %.0f GB/s"
              % (mc, nb / 1e6, rate(2, mc)), ""]
    result[name] = {"table": table, "update_us": mu, "swap_us": ms, "copy_us": mc, "buffer_bytes": nb}
    del eng
    torch.cuda.empty_cache()

parent = None
if args.parent_tree:
    here = os.path.abspath(args.tree)
    runs = {"this": [], "parent": []}
    for _ in range(3):
        for which, tree in (("this", here), ("parent", os.path.abspath(args.parent_tree))):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only", "--tree", tree, "--rounds", str(args.rounds),
                                "--steps", str(args.steps)], capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                raise SystemExit("child run on %s failed:\n%s" % (tree, r.stderr[-2000:]))
            runs[which].append({d["config"]: d for d in (json.loads(ln) for ln in r.stdout.strip().splitlines() if ln.startswith("{"))})
    parent = runs
    lines.append("the unconfigured step, this tree against a build of the parent commit, child processes in turns:")
    for name in CONFIGS:
        for which in ("this", "parent"):
            for i, r in enumerate(runs[which]):
                s = r[name]
                lines.append("  %s %-7s run %d: median %.3f ms, min %.3f, max %.3f (%d windows)" % (name, which, i, s["median_ms"], s["min_ms"], s["max_ms"], s["n"]))
        mt, mp = (np.median([r[name]["median_ms"] for r in runs[w]]) for w in ("this", "parent"))
        pm = [r[name]["median_ms"] for r in runs["parent"]]
        lo, hi = min(pm), max(pm)
        lines.append("  %s: median of medians, this - parent = %+.3f ms (%+.2f %%); the parent's own medians span %.3f .. %.3f ms from run to "
                     "run: this tree's %.3f ms %s" % (name, mt - mp, 100.0 * (mt - mp) / mp, lo, hi, mt,
                                                      "lies inside that span" if lo <= mt <= hi else
                                                      ("lies BELOW it (same launches: process-to-process noise)" if mt < lo else "lies ABOVE it")))
text = "\n".join(lines)
print(text)
print(json.dumps({"result": result, "parent": parent}))
if args.record:
    with open(args.record, "w") as f:
        f.write(text + "\n")
