#!/usr/bin/env python
"""Cost of the sampled token selection per decoded position, next to greedy decoding: cfg-2 dimensions (seq_len 200, d 128,
8 heads, dff 512, 4 layers), B = 128, the EOS stop disabled (eos = -1, max_steps = 200), at V = 1004 and V = 10004.
    python tools/sample_bench.py [--rounds R] [--tree DIR] [--greedy-only] [--json OUT.json]
    python tools/sample_bench.py --report OUT.txt [--parent PARENT.json ...] NEW.json ...
Four modes - greedy, temperature-only (T 0.8), top-k = 40, top-k = 40 with top-p = 0.9 - are timed in turn, R rounds after one
warm-up round, in one process: a decode call (host clock around the call, which ends in a device synchronise) over its 200
positions.  The call includes what every mode shares: the K|V projection of pre_decoder and the read-back of the tokens.
  --tree DIR      import sketchformer_amd from another checkout (a build of the parent commit, for the greedy figure)
  --greedy-only   that checkout has no sampled decode
  --report        gather runs of this tool (alternated with runs on the parent's build on the same machine) into the text
                  file kept under profiles/"""
import argparse
import json
import os
import sys
import time

import numpy as np

MODES = [("greedy", None), ("temperature", dict(temperature=0.8)), ("top_k_40", dict(temperature=0.8, top_k=40)),
         ("top_k_40_top_p_0.9", dict(temperature=0.8, top_k=40, top_p=0.9))]
B, L = 128, 200


def run(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sketchformer_amd import engine, synthetic
    rec = {"rounds": args.rounds, "tree": args.tree or ".", "us_per_position": {}}
    for V in (1004, 10004):
        cfg = engine.make_config(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=V, n_classes=345,
                                 lowerdim=128, dropout_rate=0.0, use_graph=False, seed=1)
        eng = engine.TrainEngine(cfg, init_seed=2)
        x, _ = synthetic.token_batch(B, L, V, 345, seed=5)
        eng.encode(x)
        modes = MODES[:1] if args.greedy_only else MODES
        times = {name: [] for name, _ in modes}
        for r in range(args.rounds + 1):
            for name, kw in modes:
                t0 = time.perf_counter()
                if kw is None:
                    got = eng.greedy_decode(None, sos=V - 2, eos=-1, max_steps=L)
                else:
                    got = eng.sample_decode(None, sos=V - 2, eos=-1, max_steps=L, seed=r, **kw)
                dt = time.perf_counter() - t0
                assert got.shape == (B, L + 1), got.shape
                if r:                                      # round 0 warms up (code objects, the captured step, attributes)
                    times[name].append(1e6 * dt / L)
        rec["us_per_position"][str(V)] = times
        del eng
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
    out = ["sampled decode: microseconds per position (one decode call / 200 positions), cfg-2 dimensions, B = 128, no EOS stop",
           "%d run(s) of this build%s, each %d rounds per mode after a warm-up round, modes interleaved"
           % (len(new), ", alternated with %d run(s) of the parent commit's build (greedy only)" % len(parent) if parent else "",
              new[0]["rounds"]), ""]
    for V in ("1004", "10004"):
        out.append("V = %s" % V)
        pooled = {name: sum((r["us_per_position"][V].get(name, []) for r in new), []) for name, _ in MODES}
        g = float(np.median(pooled["greedy"]))
        if parent:
            out.append("  %-22s %s" % ("greedy, parent commit", _stat(sum((r["us_per_position"][V]["greedy"] for r in parent), []))))
            for i, r in enumerate(parent):
                out.append("  %-22s %s" % ("  parent run %d" % (i + 1), _stat(r["us_per_position"][V]["greedy"])))
        for i, r in enumerate(new):
            out.append("  %-22s %s" % ("  greedy, run %d" % (i + 1), _stat(r["us_per_position"][V]["greedy"])))
        for name, _ in MODES:
            out.append("  %-22s %s  = %.3f x greedy" % (name, _stat(pooled[name]), np.median(pooled[name]) / g))
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
