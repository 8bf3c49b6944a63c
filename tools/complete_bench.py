#!/usr/bin/env python
"""Sketch completion at the cfg-2 dimensions, B = 128: what the cache prefill gains over stepping through the prefix.
    python tools/complete_bench.py [--reps 24] [--record profiles/complete_bench.txt] [--parent-tree DIR]
  (a) greedy completion, prefix length 100 in every row: stepwise = 1 against stepwise = 0 (the prefill)
  (b) QuickDraw-like ragged sketch lengths, every sketch cut at one half: both ways
  (c) plain skf_model_greedy_decode, for context
The variants alternate inside one process (a1 a0 b1 b0 c, repeated); every call is timed with events on the engine's stream and goes
into preallocated device buffers.  A second pass with the library's launch profiler gives the prefill launches alone.
  --parent-tree DIR   also time (c) on the package under DIR (a build of the parent commit): child processes, this tree and that one
                      in turns (the two libraries cannot share a process), two rounds each
  --plain-only        what such a child runs: (c) alone, on the package of --tree, one JSON line"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--record")
ap.add_argument("--parent-tree")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch                                           # noqa: E402
from sketchformer_amd import _lib, engine, synthetic   # noqa: E402

B, L, V = 128, 200, 1004
cfg = engine.make_config(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=V, n_classes=345,
                         lowerdim=128, dropout_rate=0.0, use_graph=False, seed=1)
eng = engine.TrainEngine(cfg, init_seed=2)
x, _ = synthetic.token_batch(B, L, V, 345, seed=5)
eng.encode(x)
eng.synchronize()
emb = eng.buffer("embedding").float().clone()
sos, eos = V - 2, V - 1
out = torch.empty(B, L + 1, dtype=torch.int64, device=eng.device)
n_out = C.c_int(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(eng.stream)
    fn()
    e1.record(eng.stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def plain():
    _lib.call("skf_model_greedy_decode", eng.handle, eng._p(emb), None, B, sos, eos, L, eng._p(out), C.byref(n_out), eng._stream())


def stats(ts):
    ts = np.asarray(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
            "spread_ms": float(np.percentile(ts, 90) - np.percentile(ts, 10)), "n": int(len(ts))}


if args.plain_only:
    for _ in range(args.warmup):
        plain()
    print(json.dumps(dict(stats([timed(plain) for _ in range(args.reps)]), columns=n_out.value)))
    sys.exit(0)

rng = np.random.RandomState(7)
prefix = torch.from_numpy(rng.randint(1, V - 3, size=(B, L)).astype(np.int64)).to(eng.device)
# QuickDraw-like lengths: most sketches are short, a few fill the row (a gamma of mean 72 cut to [8, 198]); the prefix is one half
ragged = np.clip(rng.gamma(4.0, 18.0, size=B), 8, L - 2).astype(np.int64) // 2
cases = {"a": np.full(B, 100, np.int64), "b": ragged}


def completion(lens, stepwise):
    arr = (C.c_int * B)(*[int(v) for v in lens])
    pf = _lib.SkfPrefix(tokens=prefix.data_ptr(), ld=L, len_host=arr, stepwise=stepwise)

    def call():
        _lib.call("skf_model_prefix_decode", eng.handle, eng._p(emb), None, B, sos, eos, L, eng._p(out), C.byref(n_out), C.byref(pf),
                  None, None, eng._stream())
    return call


variants = [("a_stepwise", completion(cases["a"], 1)), ("a_prefill", completion(cases["a"], 0)),
            ("b_stepwise", completion(cases["b"], 1)), ("b_prefill", completion(cases["b"], 0)), ("c_plain_greedy", plain)]
results = {}
for name, fn in variants:                              # the two ways of a case give the same tokens
    fn()
    eng.synchronize()
    results[name] = out[:, :n_out.value].clone()
assert torch.equal(results["a_stepwise"], results["a_prefill"]) and torch.equal(results["b_stepwise"], results["b_prefill"])
for _ in range(args.warmup):
    for _, fn in variants:
        fn()
times = {name: [] for name, _ in variants}
for _ in range(args.reps):
    for name, fn in variants:
        times[name].append(timed(fn))
table = {name: stats(ts) for name, ts in times.items()}

# the launches alone (the library's profiler: events around every launch scope)
lib = _lib.load()
prof = {}
for name in ("a_stepwise", "a_prefill", "b_prefill"):
    fn = dict(variants)[name]
    lib.skf_profiler_enable(1)
    for _ in range(3):
        fn()
    eng.synchronize()
    buf = C.create_string_buffer(1 << 16)
    _lib.check(lib.skf_profiler_report(buf, len(buf)), "skf_profiler_report")
    lib.skf_profiler_enable(0)
    prof[name] = {r["tag"]: {"launch_scopes_per_call": r["count"] / 3.0, "ms_per_call": r["ms"] / 3.0} for r in json.loads(buf.value.decode())
                  if r["tag"].startswith("decode_")}

parent = None
if args.parent_tree:
    here = os.path.abspath(args.tree)
    runs = {"this": [], "parent": []}
    for _ in range(2):
        for which, tree in (("this", here), ("parent", os.path.abspath(args.parent_tree))):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", tree, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                raise SystemExit("child run on %s failed:\n%s" % (tree, r.stderr[-2000:]))
            runs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
    parent = runs

gain = table["a_stepwise"]["median_ms"] - table["a_prefill"]["median_ms"]
accepted = gain > table["a_stepwise"]["spread_ms"]
lines = ["tools/complete_bench.py on %s: cfg-2 dimensions (4 layers, 8 heads, d 128, dff 512, V 1004), B = 128, seq_len 200, random weights"
         % torch.cuda.get_device_name(0),
         "events on the engine's stream around the C entry, %d warm-up rounds, %d repetitions, variants in turns (a1 a0 b1 b0 c)"
         % (args.warmup, args.reps),
         "every call: expander + cross K|V of 4 layers, then the positions up to column 200 (random weights draw no EOS)", "",
         "%-16s %10s %10s %10s %14s" % ("variant", "median ms", "min ms", "max ms", "p90 - p10 ms")]
for name, _ in variants:
    s = table[name]
    lines.append("%-16s %10.3f %10.3f %10.3f %14.3f" % (name, s["median_ms"], s["min_ms"], s["max_ms"], s["spread_ms"]))
lines += ["", "a: prefix length 100 in every row; b: ragged lengths (gamma of mean 72, cut to [8, 198]) halved: prefix %d .. %d, mean %.1f"
          % (ragged.min(), ragged.max(), ragged.mean()),
          "a: the prefill saves %.3f ms of the stepwise median, %.1f x the stepwise spread (p90 - p10): acceptance %s"
          % (gain, gain / max(table["a_stepwise"]["spread_ms"], 1e-9), "met" if accepted else "NOT met"),
          "b: the prefill saves %.3f ms" % (table["b_stepwise"]["median_ms"] - table["b_prefill"]["median_ms"]), "",
          "launch scopes alone (library profiler, mean of 3 calls; decode_prefill = the 4 layer launches of one call):"]
for name, tags in prof.items():
    for tag, r in sorted(tags.items()):
        lines.append("  %-12s %-22s %8.1f scopes / call %10.3f ms / call" % (name, tag, r["launch_scopes_per_call"], r["ms_per_call"]))
if parent:
    lines += ["", "plain greedy_decode of 128 x 200, this tree against a build of the parent commit, child processes in turns:"]
    for which in ("this", "parent"):
        for i, r in enumerate(parent[which]):
            lines.append("  %-7s run %d: median %.3f ms, min %.3f, max %.3f, p90 - p10 %.3f (%d repetitions)"
                         % (which, i, r["median_ms"], r["min_ms"], r["max_ms"], r["spread_ms"], r["n"]))
    mt, mp = (np.mean([r["median_ms"] for r in parent[w]]) for w in ("this", "parent"))
    rr = max(abs(parent[w][0]["median_ms"] - parent[w][1]["median_ms"]) for w in ("this", "parent"))
    lines.append("  this - parent = %+.3f ms (%+.2f %%); run-to-run difference of one build's medians: up to %.3f ms"
                 % (mt - mp, 100.0 * (mt - mp) / mp, rr))
text = "\n".join(lines)
print(text)
print(json.dumps({"table": table, "profile": prof, "parent": parent, "accepted": bool(accepted)}))
if args.record:
    with open(args.record, "w") as f:
        f.write(text + "\n")
