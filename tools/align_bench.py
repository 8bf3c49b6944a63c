#!/usr/bin/env python
"""Times the sequence-alignment kernels (ops.edit_distance / ops.dtw_distance over skf_align.hip) at the sizes a user runs: paired,
B = 128 pairs of L = 200 (a validation batch against its reconstructions), and cross, 256 queries x 4096 gallery rows of L = 200
(the distance matrix of a retrieval baseline), for both distances - and, for the paired case, the host restatement of
tests/align_reference.py on the same inputs on the same machine.

Device times are HIP events around groups of --group calls after a warm-up, the median over --repeats, divided by the group
size; a cell is one entry of a pair's La x Lb table, so cells per second = pairs * L * L / time.  The host figure is wall clock
for all B pairs.  The results of the timed inputs are checked against the restatement first (paired: all pairs; cross: a few
entries).  Out goes ONE JSON line; with --record also a text record (profiles/align_bench.txt).

    python tools/align_bench.py
    python tools/align_bench.py --pairs 128 --length 200 --queries 256 --gallery 4096 --record profiles/align_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, group, repeats, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) / group * 1e3)
    return round(statistics.median(us), 2), [round(v, 2) for v in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--gallery", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--cross-group", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import align_reference as ref
    from sketchformer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("align_bench needs the GPU: nothing here is measured on the host alone")
    B, L, Q, G = args.pairs, args.length, args.queries, args.gallery
    rng = np.random.RandomState(0)
    N = max(B, G)

    def ids(n):
        return rng.randint(1, args.vocab + 1, size=(n, L)).astype(np.int64)

    def walks(n):                                                  # pen positions of a random walk inside the unit box
        return np.clip(np.cumsum(rng.randn(n, L, 2) * 0.05, axis=1), -1, 1).astype(np.float32)

    tok_a, tok_b, xy_a, xy_b = ids(max(B, Q)), ids(N), walks(max(B, Q)), walks(N)
    dev = lambda a: torch.from_numpy(a).cuda()                      # noqa: E731
    full = torch.full((max(B, Q, G),), L, dtype=torch.int32, device="cuda")
    lens = lambda n: full[:n]                                       # noqa: E731  (made once: a timed call is the launch alone)
    d_tok_a, d_tok_b, d_xy_a, d_xy_b = dev(tok_a), dev(tok_b), dev(xy_a), dev(xy_b)
    out = {"pairs": B, "length": L, "queries": Q, "gallery": G, "device": torch.cuda.get_device_name(0)}

    runs = {
        "edit_paired": (lambda: ops.edit_distance(d_tok_a[:B], d_tok_b[:B], lens(B), lens(B)), B, args.group),
        "dtw_paired": (lambda: ops.dtw_distance(d_xy_a[:B], lens(B), d_xy_b[:B], lens(B)), B, args.group),
        "edit_cross": (lambda: ops.edit_distance(d_tok_a[:Q], d_tok_b[:G], lens(Q), lens(G), cross=True), Q * G, args.cross_group),
        "dtw_cross": (lambda: ops.dtw_distance(d_xy_a[:Q], lens(Q), d_xy_b[:G], lens(G), cross=True), Q * G, args.cross_group),
    }
    # the timed inputs give the restatement's results
    t0 = time.perf_counter()
    want_edit = np.array([ref.edit_distance_ref(tok_a[i], tok_b[i]) for i in range(B)])
    host_edit_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_dtw = np.array([ref.dtw_ref(xy_a[i], xy_b[i]) for i in range(B)], np.float32)
    host_dtw_s = time.perf_counter() - t0
    assert np.array_equal(runs["edit_paired"][0]().cpu().numpy(), want_edit)
    assert np.array_equal(runs["dtw_paired"][0]().cpu().numpy().view(np.uint32), want_dtw.view(np.uint32))
    ce, cd = runs["edit_cross"][0]().cpu().numpy(), runs["dtw_cross"][0]().cpu().numpy()
    for i, j in ((0, 0), (Q - 1, G - 1), (Q // 2, 1), (3, G // 2)):
        assert ce[i, j] == ref.edit_distance_ref(tok_a[i], tok_b[j])
        assert cd[i, j].tobytes() == ref.dtw_ref(xy_a[i], xy_b[j]).tobytes()
    out["checked"] = "paired: all pairs equal to the host restatement (DTW bit for bit); cross: 4 entries each"

    for name, (fn, pairs, group) in runs.items():
        us, all_us = timed(fn, group, args.repeats, args.warmup)
        out[name] = {"us": us, "repeats_us": all_us, "pairs": pairs, "cells_per_s": round(pairs * L * L / (us * 1e-6), 1)}
    if not args.no_host:
        out["host_edit_paired_s"] = round(host_edit_s, 4)
        out["host_dtw_paired_s"] = round(host_dtw_s, 4)
        out["host_edit_over_device"] = round(host_edit_s / (out["edit_paired"]["us"] * 1e-6), 1)
        out["host_dtw_over_device"] = round(host_dtw_s / (out["dtw_paired"]["us"] * 1e-6), 1)
    print(json.dumps(out))
    if args.record:
        with open(args.record, "w") as f:
            f.write("tools/align_bench.py on %s: HIP events, median of %d repeats (groups of %d paired / %d cross calls, %d warm-up calls)\n"
                    % (out["device"], args.repeats, args.group, args.cross_group, args.warmup))
            f.write("%s\n\n" % out["checked"])
            f.write("%-12s %10s %14s %12s   %s\n" % ("case", "pairs", "time (us)", "Gcells/s", "repeats (us)"))
            for name in runs:
                r = out[name]
                f.write("%-12s %10d %14.2f %12.2f   %s\n" % (name, r["pairs"], r["us"], r["cells_per_s"] / 1e9, r["repeats_us"]))
            f.write("\npaired = %d pairs of L = %d; cross = %d x %d rows of L = %d; a cell is one entry of a pair's L x L table\n" % (B, L, Q, G, L))
            if not args.no_host:
                f.write("host restatement (tests/align_reference.py), the same %d pairs, wall clock: edit %.3f s (%.0f x the device call), "
                        "dtw %.3f s (%.0f x)\n" % (B, host_edit_s, out["host_edit_over_device"], host_dtw_s, out["host_dtw_over_device"]))
            build = os.path.join(ROOT, "profiles", "align_build.txt")
            if os.path.exists(build):                              # registers and LDS of the kernels as compiled
                with open(build) as b:
                    f.write("\n" + b.read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
