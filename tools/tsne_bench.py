#!/usr/bin/env python
"""Times the device t-SNE (ops.tsne_affinities / ops.tsne_step over skf_tsne.hip, projection.tsne) at the metric's shape
(N = 1000, d = 256) and at the kernels' limit (N = 8192), and, for scale, this repository's float64 numpy oracle
(tests/tsne_reference.py) per iteration at N = 1000 on the CPU.

Per size: the affinities in ms (HIP events around the call, median over --repeats); one iteration in us (events around groups of
--group iterations, median, divided by the group size); the split of an iteration between its two launches from the library's
launch profiler (events around every launch, so each figure carries a few us of its own); the pair pass against the time its read
of P costs at the measured HBM copy rate (6.29 TB/s, MI355X_MICROARCH) - the floor where P does not stay in cache; and a whole
1000-iteration fit through projection.tsne, wall clock, affinities and transfers included.  Out goes ONE JSON line.

    python tools/tsne_bench.py
    python tools/tsne_bench.py --sizes 1000 --no-oracle
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.29e12


def profile_split(ops, P, Y, U, gains, n):
    lib = ops._lib.load()
    lib.skf_profiler_enable(1)
    for _ in range(n):
        ops.tsne_step(P, Y, U, gains, 1.0, 0.8, 200.0)
    buf = C.create_string_buffer(1 << 16)
    ops._lib.check(lib.skf_profiler_report(buf, len(buf)), "skf_profiler_report")
    lib.skf_profiler_enable(0)
    return {r["tag"]: r["ms"] / r["count"] * 1e3 for r in json.loads(buf.value.decode())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 8192])
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--group", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--fit-iters", type=int, default=1000)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from sketchformer_amd import ops, projection
    import tsne_reference as ref
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    out = {"tool": "tsne_bench", "d": args.d, "perplexity": args.perplexity, "group": args.group, "repeats": args.repeats, "sizes": []}
    for N in args.sizes:
        x_np = ref.blobs(N, args.d, 10, 0, 2.0)[0]
        x = torch.from_numpy(x_np).to(dev)
        P = ops.tsne_new_affinities(N, dev)
        ws = torch.empty(ops._lib.load().skf_tsne_workspace_bytes(N), dtype=torch.uint8, device=dev)
        ops.tsne_affinities(x, args.perplexity, out=P, workspace=ws)
        torch.cuda.synchronize()
        aff = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); ops.tsne_affinities(x, args.perplexity, out=P, workspace=ws); b.record()
            torch.cuda.synchronize()
            aff.append(a.elapsed_time(b))
        Y = torch.from_numpy(ref.random_init(N, 14)).to(dev)
        U, gains = torch.zeros_like(Y), torch.ones_like(Y)

        def steps(n, ex=1.0, mom=0.8):
            for _ in range(n):
                ops.tsne_step(P, Y, U, gains, ex, mom, 200.0, workspace=ws)

        steps(args.warmup, 12.0, 0.5)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); steps(args.group); b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) / args.group * 1e3)
        split = profile_split(ops, P, Y, U, gains, args.group)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); kl = ops.tsne_kl(P, Y, workspace=ws); b.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yfit, klfit = projection.tsne(x_np, perplexity=args.perplexity, n_iter=args.fit_iters, return_kl=True)
        fit_s = time.perf_counter() - t0
        floor_us = 4.0 * N * N / HBM_BYTES_PER_S * 1e6
        med = statistics.median(us)
        out["sizes"].append({
            "N": N, "affinities_ms": round(statistics.median(aff), 3), "affinities_ms_all": [round(v, 3) for v in aff],
            "us_per_iteration": round(med, 2), "us_per_iteration_all": [round(v, 2) for v in us],
            "us_per_launch": round(med / 2.0, 2),
            "profiled_pair_us": round(split.get("tsne_pair", float("nan")), 2),
            "profiled_update_us": round(split.get("tsne_update", float("nan")), 2),
            "p_read_floor_us": round(floor_us, 2), "pair_over_floor": round(split.get("tsne_pair", float("nan")) / floor_us, 3),
            "pairs_per_s": round(float(N) * N / (med * 1e-6), 1), "kl_ms": round(a.elapsed_time(b), 3), "kl_after_bench_steps": float(kl.cpu()[0]),
            "fit_iterations": args.fit_iters, "fit_wall_s": round(fit_s, 3), "fit_kl": klfit, "fit_finite": bool(np.isfinite(yfit).all())})
        del P, x, Y, U, gains
    if not args.no_oracle:
        N = 1000
        xo = ref.blobs(N, args.d, 10, 0, 2.0)[0]
        t0 = time.perf_counter()
        P64, _ = ref.affinities(ref.distances(xo), args.perplexity)
        t_aff = time.perf_counter() - t0
        Y = ref.random_init(N, 14).astype(np.float64)
        Uo, go = np.zeros_like(Y), np.ones_like(Y)
        t0 = time.perf_counter()
        for _ in range(5):
            _, _, Y, Uo, go = ref.step(P64, Y, Uo, go, 12.0, 0.5, 200.0)
        out["oracle_cpu"] = {"N": N, "affinities_s": round(t_aff, 3), "s_per_iteration": round((time.perf_counter() - t0) / 5, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
