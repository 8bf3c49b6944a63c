#!/usr/bin/env python
"""What gradient clipping costs a train step, at the cfg-2 (fp32, B = 128) and cfg-5 (bf16, B = 8) dimensions.
    python tools/clip_bench.py [--rounds 6] [--steps 20] [--record profiles/grad_clip_bench.txt] [--parent-tree DIR]
  (a) ms/step of train_step with clipping off, global_clipnorm, clipnorm (per variable), clipvalue and monitor only.  One engine per
      config; the variants alternate inside one process (off global per-variable clipvalue monitor, repeated `rounds` times), every
      window is `steps` steps between a device synchronise and the next, after two warm-up steps of that variant.  Thresholds are
      small enough to be active on every step.
  (b) the two norm launches alone on the config's gradient buffer, and their bytes/s beside a device copy of as many floats in the
      same run (in turns).
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

CONFIGS = {
    "cfg2": dict(batch=128, kw=dict(seq_len=200, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=1004, n_classes=345, lowerdim=256,
                                    dropout_rate=0.1, seed=1234, act_dtype="f32")),
    "cfg5": dict(batch=8, kw=dict(seq_len=512, d_model=512, num_heads=8, dff=2048, num_layers=8, vocab_size=1004, n_classes=345, lowerdim=256,
                                  dropout_rate=0.1, seed=1234, act_dtype="bf16")),
}
VARIANTS = [("off", {}), ("global", dict(global_clipnorm=1e-3)), ("per_variable", dict(clipnorm=1e-4)), ("clipvalue", dict(clipvalue=1e-6)),
            ("monitor", dict(monitor=True))]


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


lines = ["tools/clip_bench.py on %s: train_step (forward, backward, optimizer) with synthetic batches, dropout 0.1, eager launches"
         % torch.cuda.get_device_name(0),
         "windows of %d steps between two device synchronises, 2 warm-up steps of the variant first, variants in turns, %d rounds"
         % (args.steps, args.rounds), ""]
result = {}
for name in CONFIGS:
    eng, x, y = build(name)
    window(eng, x, y, args.steps, warmup=5)
    times = {v: [] for v, _ in VARIANTS}
    seen = {}
    for _ in range(args.rounds):
        for v, settings in VARIANTS:
            eng.set_gradient_clip(**settings)
            times[v].append(window(eng, x, y, args.steps))
            if settings:
                seen[v] = eng.gradient_stats()
    eng.set_gradient_clip()
    table = {v: stats(ts) for v, ts in times.items()}
    off = table["off"]
    lines += ["%s: B = %d, %s, %d parameters in %d variables, %d chunks of %d elements"
              % (name, CONFIGS[name]["batch"], CONFIGS[name]["kw"]["act_dtype"], sum(e["rows"] * e["cols"] for e in eng.entries), len(eng.entries),
                 ops.segment_plan(eng.entries, eng.device).n_chunks, ops.SEGMENT_CHUNK),
              "  %-13s %10s %10s %10s %16s" % ("variant", "median ms", "min ms", "max ms", "median - off")]
    for v, _ in VARIANTS:
        s = table[v]
        lines.append("  %-13s %10.3f %10.3f %10.3f %+10.3f ms (%+.2f %%)" % (v, s["median_ms"], s["min_ms"], s["max_ms"], s["median_ms"] - off["median_ms"],
                                                                              100.0 * (s["median_ms"] - off["median_ms"]) / off["median_ms"]))
    lines.append("  spread of the off windows (max - min): %.3f ms; last step: global norm %.4g -> scale %.4g (global), %d of %d variables scaled "
                 "(per variable)" % (off["max_ms"] - off["min_ms"], seen["global"]["global_norm"], seen["global"]["scale"],
                                     sum(s < 1.0 for s in seen["per_variable"]["scales"].values()), len(eng.entries)))
    # (b) the norm launches alone, beside a device copy of as many floats
    plan = ops.segment_plan(eng.entries, eng.device)
    g = eng.grads
    st = ops.new_segment_stats(plan)
    ws = torch.empty(int(eng.lib.skf_segment_norms_workspace_bytes(plan.n_entries, plan.n_chunks)) + 256, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(g)
    norms = lambda: ops.segment_norms(g, plan, mode="global", threshold=1e-3, stats=st, workspace=ws)      # noqa: E731
    copy = lambda: dst.copy_(g)                                                                          # noqa: E731
    for fn in (norms, copy):
        events(fn, 20)
    us = {"norms": [], "copy": []}
    for _ in range(args.rounds):
        us["norms"].append(events(norms, 50))
        us["copy"].append(events(copy, 50))
    n_read = 4 * sum(e["rows"] * e["cols"] for e in eng.entries)
    mn, mc = float(np.median(us["norms"])), float(np.median(us["copy"]))
    lines += ["  norm launches alone (sum of squares + finish, 50 back-to-back calls per window): %.1f us per call, %.2f MB read -> %.0f GB/s"
              % (mn, n_read / 1e6, n_read / (mn * 1e-6) / 1e9),
              "  device copy of the flat buffer in the same run: %.1f us per call, %.2f MB read + as much written -> %.0f GB/s"
              % (mc, 4 * g.numel() / 1e6, 2 * 4 * g.numel() / (mc * 1e-6) / 1e9), ""]
    result[name] = {"table": table, "norms_us": mn, "copy_us": mc, "bytes_read": n_read}
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
        spread = max(pm) - min(pm)
        lines.append("  %s: median of medians, this - parent = %+.3f ms (%+.2f %%); the parent's own medians span %.3f ms from run to run: "
                     "this tree's off step %s" % (name, mt - mp, 100.0 * (mt - mp) / mp, spread,
                                                  "is inside the parent's spread" if abs(mt - mp) <= spread else
                                                  ("is FASTER than the parent by more than its spread (same launches: process-to-process noise)"
                                                   if mt < mp else "is SLOWER than the parent by more than its spread")))
text = "\n".join(lines)
print(text)
print(json.dumps({"result": result, "parent": parent}))
if args.record:
    with open(args.record, "w") as f:
        f.write(text + "\n")
