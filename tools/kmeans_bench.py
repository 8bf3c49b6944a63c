#!/usr/bin/env python
"""Times one Lloyd iteration of the device k-means (ops.kmeans_step: clear + assign/accumulate + update, skf_kmeans.hip) at the size
of the token dictionary - N = 5 M points, K = 1000 centres - and, for scale, sklearn's Lloyd on the CPU threads of the box from the
same initial centres at N = 500 k (the reference's create_token_dict.py runs sklearn at 5 M).

Device time: HIP events around groups of --group iterations (one iteration is too short a window), median over --repeats groups
after --warmup iterations, divided by the group size; tol is off so every iteration does its full work.  Out goes ONE JSON line:
ms per iteration, point-centre pairs per second, the share of the fp32 vector rate that the loop's instruction count predicts
(DESIGN.md section 3g), and the sklearn leg's seconds per iteration.

    python tools/kmeans_bench.py
    python tools/kmeans_bench.py --N 500000 --no-sklearn
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9      # MI355X: 256 CUs x 4 SIMD-32 at 2.4 GHz (157.3 TF = two flops per lane-op)
VALU_PER_PAIR = 229.0 / 32.0                    # shipped ISA of kmeans_assign_kernel: 229 VALU per 4 centres x 8 points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=5000000)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--group", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sklearn-N", type=int, default=500000)
    ap.add_argument("--sklearn-iters", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    from sketchformer_amd import kmeans, ops
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    # offsets like the dictionary's: most of them short, a heavy tail of pen-lift jumps
    rs = np.random.RandomState(args.seed)
    pts_np = (rs.standard_t(3, size=(args.N, 2)) * 0.03).clip(-1, 1).astype(np.float32)
    pts = torch.from_numpy(pts_np).to(dev)
    c0 = kmeans.init_centers(pts_np, args.K, "random", seed=args.seed)
    centers = torch.from_numpy(c0).to(dev)
    state = ops.new_kmeans_state(dev)
    e = ops.kmeans_scale_exp(float(pts.abs().max()))
    labels = torch.empty(args.N, dtype=torch.int32, device=dev)
    counts = torch.empty(args.K, dtype=torch.int32, device=dev)
    ws = torch.empty(ops._lib.load().skf_kmeans_workspace_bytes(args.N, args.K), dtype=torch.uint8, device=dev)

    def steps(n):
        for _ in range(n):
            ops.kmeans_step(pts, centers, state, e, -1.0, labels=labels, counts=counts, workspace=ws)

    steps(args.warmup)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); steps(args.group); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.group)
    st = ops.read_kmeans_state(state)
    med = statistics.median(ms)
    pairs = float(args.N) * args.K
    model_ms = pairs * VALU_PER_PAIR / VALU_LANE_OPS_PER_S * 1e3
    out = {"tool": "kmeans_bench", "N": args.N, "K": args.K, "group": args.group, "repeats": args.repeats,
           "ms_per_iteration": round(med, 4), "ms_per_iteration_all": [round(x, 4) for x in ms],
           "pairs_per_s": round(pairs / (med * 1e-3), 1), "model_ms_per_iteration": round(model_ms, 4),
           "model_over_measured": round(model_ms / med, 4), "iterations": st["iterations"], "inertia": st["inertia"]}
    if not args.no_sklearn:
        from sklearn.cluster import KMeans
        n = min(args.sklearn_N, args.N)
        t0 = time.perf_counter()
        km = KMeans(n_clusters=args.K, init=c0, n_init=1, max_iter=args.sklearn_iters, tol=0.0, algorithm="lloyd").fit(pts_np[:n])
        dt = time.perf_counter() - t0
        out.update({"sklearn_N": n, "sklearn_iterations": int(km.n_iter_), "sklearn_s_per_iteration": round(dt / max(int(km.n_iter_), 1), 4),
                    "sklearn_pairs_per_s": round(float(n) * args.K * int(km.n_iter_) / dt, 1),
                    "sklearn_threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
