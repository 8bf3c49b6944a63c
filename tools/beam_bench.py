#!/usr/bin/env python
"""Cost of beam-search decoding per position, next to greedy decoding: cfg-2 dimensions (seq_len 200, d 128, 8 heads, dff 512,
4 layers, V 1004), B = 128, the EOS stop disabled (eos = -1, max_steps = 200).
    python tools/beam_bench.py [--rounds R] [--tree DIR] [--greedy-only] [--json OUT.json]
    python tools/beam_bench.py --report OUT.txt [--parent PARENT.json ...] NEW.json ...
Three measurements:
  1. greedy on the parent commit's build against greedy on this one (no greedy instruction changed: the two must lie within the
     run-to-run spread that the alternation shows).  Run the tool 5 times on each build, alternating, on one machine:
         for i in 1 2 3 4 5; do python tools/beam_bench.py --tree PARENT --greedy-only --json p$i.json;
                                python tools/beam_bench.py --json n$i.json; done
         python tools/beam_bench.py --report profiles/beam_decode_bench.txt --parent p1.json ... --parent p5.json n1.json ... n5.json
  2. beam search with W = 1, 4, 8 per position against this build's greedy at the same B: the beam call decodes B / W sketches in
     the same B rows, so a position costs the same B workgroups plus the merge launch.  Host clock around the call, which ends in a
     device synchronise; modes interleaved, R rounds after one warm-up round.
  3. the split between the position kernel and the advance kernel: one further beam call per width under the library's launch
     profiler (skf_profiler_enable: events around every launch, so this call is not among the timed ones).
  --tree DIR      import sketchformer_amd from another checkout (a build of the parent commit, for the greedy figure)
  --greedy-only   that checkout has no beam decode
  --report        gather the alternated runs into the text file kept under profiles/"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

WIDTHS = (1, 4, 8)
B, L, V = 128, 200, 1004
SPLIT_TAGS = ("decode_position_beam", "beam_advance")


def _split(eng, lib, emb, W):
    """microseconds per launch of the two kernels of a beam position, from the launch profiler"""
    import torch
    torch.cuda.synchronize()
    lib.skf_profiler_enable(1)
    eng.beam_decode(emb[:B // W], sos=V - 2, eos=-1, max_steps=L, beam_width=W)
    torch.cuda.synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.skf_profiler_report(buf, len(buf))
    lib.skf_profiler_enable(0)
    rows = {r["tag"]: r for r in json.loads(buf.value.decode())}
    return {t: (1e3 * rows[t]["ms"] / rows[t]["count"] if t in rows and rows[t]["count"] else None) for t in SPLIT_TAGS}


def run(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sketchformer_amd import _lib, engine, synthetic
    cfg = engine.make_config(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=V, n_classes=345,
                             lowerdim=128, dropout_rate=0.0, use_graph=False, seed=1)
    eng = engine.TrainEngine(cfg, init_seed=2)
    x, _ = synthetic.token_batch(B, L, V, 345, seed=5)
    eng.encode(x)
    emb = eng.buffer("embedding").float().clone()
    modes = [("greedy", None)] + ([] if args.greedy_only else [("beam_%d" % W, W) for W in WIDTHS])
    times = {name: [] for name, _ in modes}
    for r in range(args.rounds + 1):
        for name, W in modes:
            t0 = time.perf_counter()
            if W is None:
                got = eng.greedy_decode(emb, sos=V - 2, eos=-1, max_steps=L)
                want = (B, L + 1)
            else:
                got = eng.beam_decode(emb[:B // W], sos=V - 2, eos=-1, max_steps=L, beam_width=W)[0]
                want = (B // W, W, L + 1)
            dt = time.perf_counter() - t0
            assert got.shape == want, (got.shape, want)
            if r:                                          # round 0 warms up (code objects, attributes)
                times[name].append(1e6 * dt / L)
    rec = {"rounds": args.rounds, "tree": args.tree or ".", "us_per_position": times, "split_us": {}}
    if not args.greedy_only:
        lib = _lib.load()
        for W in WIDTHS:
            rec["split_us"][str(W)] = _split(eng, lib, emb, W)
    print(json.dumps(rec))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


def _stat(v):
    v = np.asarray(v, dtype=np.float64)
    return "median %7.1f  min %7.1f  max %7.1f  (n=%d)" % (np.median(v), v.min(), v.max(), len(v))


def report(args):
    new = [json.load(open(p)) for p in args.runs]
    parent = [json.load(open(p)) for p in args.parent]
    out = ["beam-search decode: microseconds per position (one decode call / 200 positions), cfg-2 dimensions, V = 1004, B = 128 rows, "
           "no EOS stop",
           "%d run(s) of this build%s, each %d rounds per mode after a warm-up round, modes interleaved"
           % (len(new), ", alternated with %d run(s) of the parent commit's build (greedy only)" % len(parent) if parent else "",
              new[0]["rounds"]), ""]
    names = ["greedy"] + ["beam_%d" % W for W in WIDTHS]
    pooled = {n: sum((r["us_per_position"].get(n, []) for r in new), []) for n in names}
    g = float(np.median(pooled["greedy"]))
    out.append("1. greedy, parent commit against this build")
    if parent:
        pp = sum((r["us_per_position"]["greedy"] for r in parent), [])
        out.append("  %-22s %s" % ("greedy, parent commit", _stat(pp)))
        for i, r in enumerate(parent):
            out.append("  %-22s %s" % ("  parent run %d" % (i + 1), _stat(r["us_per_position"]["greedy"])))
    out.append("  %-22s %s" % ("greedy, this build", _stat(pooled["greedy"])))
    for i, r in enumerate(new):
        out.append("  %-22s %s" % ("  run %d" % (i + 1), _stat(r["us_per_position"]["greedy"])))
    if parent:
        meds = [float(np.median(r["us_per_position"]["greedy"])) for r in new + parent]
        out.append("  medians: this build / parent = %.4f; run-to-run spread of the per-run medians (max - min) / median = %.4f"
                   % (g / np.median(pp), (max(meds) - min(meds)) / np.median(meds)))
    out += ["", "2. beam search per position (B / W sketches in the same 128 rows) against this build's greedy"]
    for n in names[1:]:
        if pooled[n]:
            out.append("  %-22s %s  = %.3f x greedy" % (n, _stat(pooled[n]), np.median(pooled[n]) / g))
    out += ["", "3. the two launches of a beam position (launch profiler, microseconds per launch, median over the runs)"]
    for W in WIDTHS:
        vals = {t: [r["split_us"][str(W)][t] for r in new if r.get("split_us", {}).get(str(W), {}).get(t) is not None] for t in SPLIT_TAGS}
        if all(vals.values()):
            p, a = float(np.median(vals[SPLIT_TAGS[0]])), float(np.median(vals[SPLIT_TAGS[1]]))
            out.append("  W = %d: position kernel %7.1f   advance kernel %6.1f   (advance = %.1f %% of the two)" % (W, p, a, 100 * a / (p + a)))
    out.append("")
    text = "\n".join(out)
    print(text)
    with open(args.report, "w") as f:
        f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tree", default="")
    ap.add_argument("--greedy-only", action="store_true")
    ap.add_argument("--json", default="")
    ap.add_argument("--report", default="")
    ap.add_argument("--parent", action="append", default=[])
    ap.add_argument("runs", nargs="*")
    a = ap.parse_args()
    report(a) if a.report else run(a)
