#!/usr/bin/env python
"""Times ops.knn_topk (skf_knn_topk_f32: scores on the matrix cores, running top k in LDS, nothing Q x G in HBM) against the same
search composed from torch on the same device, in one process, on the same seeded inputs:

    blocked  queries[i:i+B] @ gallery.T  ->  + |g|^2 - 2 (.) + |q|^2  ->  torch.topk(largest=False, sorted=True)

The torch composition materialises a (B, G) score block in HBM and runs a separate selection pass over it; it is the baseline,
not the code under test.  Repeats alternate between the two; the medians, their ratio (torch / fused, >= 1 = the fused kernel is
at least as fast) and the achieved rate of the algorithmic 2 Q G d flops go out as ONE JSON line.

    python tools/knn_bench.py --Q 100000 --G 100000 --d 128 --k 100
    python tools/knn_bench.py --Q 4096 --G 862500 --d 128 --k 100
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=100000)
    ap.add_argument("--G", type=int, default=100000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--classes", type=int, default=345)
    ap.add_argument("--spread", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-block", type=int, default=4096, help="query rows per score block of the torch composition")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from sketchformer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    centres = torch.randn(args.classes, args.d, device=dev, generator=gen)
    gallery = centres[torch.randint(0, args.classes, (args.G,), device=dev, generator=gen)] + args.spread * torch.randn(args.G, args.d, device=dev, generator=gen)
    queries = centres[torch.randint(0, args.classes, (args.Q,), device=dev, generator=gen)] + args.spread * torch.randn(args.Q, args.d, device=dev, generator=gen)

    def fused():
        return ops.knn_topk(queries, gallery, args.k)

    def composed():
        gn = (gallery * gallery).sum(1)
        idx = torch.empty(args.Q, args.k, dtype=torch.int64, device=dev)
        dist = torch.empty(args.Q, args.k, dtype=torch.float32, device=dev)
        for i in range(0, args.Q, args.torch_block):
            q = queries[i:i + args.torch_block]
            s = torch.addmm(gn[None, :].expand(len(q), -1), q, gallery.t(), alpha=-2.0)
            s += (q * q).sum(1)[:, None]
            v, j = torch.topk(s, args.k, dim=1, largest=False, sorted=True)
            idx[i:i + len(q)] = j
            dist[i:i + len(q)] = v
        return idx, dist

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    for _ in range(args.warmup):
        timed(fused); timed(composed)
    t_fused, t_torch = [], []
    for _ in range(args.repeats):
        ms, (fi, fd) = timed(fused); t_fused.append(ms)
        ms, (ti, td) = timed(composed); t_torch.append(ms)
    agree = float((fi.long() == ti).float().mean())                 # rankings differ only where fp32 rounding reorders near-ties
    mf, mt = statistics.median(t_fused), statistics.median(t_torch)
    flops = 2.0 * args.Q * args.G * args.d
    print(json.dumps({
        "tool": "knn_bench", "Q": args.Q, "G": args.G, "d": args.d, "k": args.k, "classes": args.classes, "spread": args.spread,
        "repeats": args.repeats, "torch_block": args.torch_block,
        "fused_ms": round(mf, 3), "torch_ms": round(mt, 3), "fused_ms_all": [round(x, 3) for x in t_fused],
        "torch_ms_all": [round(x, 3) for x in t_torch], "ratio_torch_over_fused": round(mt / mf, 3),
        "fused_tflops": round(flops / mf / 1e9, 2), "torch_tflops": round(flops / mt / 1e9, 2),
        "fused_frac_fp32_mfma_peak": round(flops / (mf * 1e-3) / FP32_MFMA_PEAK, 4),
        "index_agreement": round(agree, 6), "max_abs_distance_diff": float((fd - td).abs().max()),
    }))


if __name__ == "__main__":
    main()
