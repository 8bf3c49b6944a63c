#!/usr/bin/env python
"""Times the device rasterizer (ops.sketch_points + ops.rasterize over skf_raster.hip) at a user's size - 128 sketches of 200
points drawn at 256 x 256 and at 64 x 64 - and, for context, the host path the experiments draw their grids with
(experiments/sampled_reconstructions.py: write_grid_png, matplotlib, one polyline at a time) on the same sketches.

Per canvas: the two launches separately and together in us (HIP events around groups of --group calls, median over --repeats,
divided by the group size: at these sizes that is the rate at which the host gets launches out), each launch on its own from the
library's launch profiler, the overlap score of the batch against itself, and the segment-pixel pairs per second the raster
launch gets through counted BEFORE culling (B * n * H * W: what a kernel without the tile cull would have to visit).  The host
figure is wall clock for one PNG of all sketches.  Out goes ONE JSON line.

    python tools/raster_bench.py
    python tools/raster_bench.py --sketches 128 --points 200 --sizes 256 64 --no-host
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sketches(B, n, seed=0):
    """(B, n, 3) float32 stroke-3 random walks: steps of ~1/40 of the unit box, a pen lift every ten points or so"""
    import numpy as np
    rng = np.random.RandomState(seed)
    s = np.zeros((B, n, 3), dtype=np.float32)
    s[:, :, :2] = rng.randn(B, n, 2) * 0.025
    s[:, :, 2] = rng.rand(B, n) < 0.1
    return s


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


def profiled(ops, fn, n):
    """us per launch from the library's launch profiler (events around every launch, so each figure carries a few us of its own
    but none of the host's time between two launches)"""
    import ctypes as C
    lib = ops._lib.load()
    lib.skf_profiler_enable(1)
    for _ in range(n):
        fn()
    buf = C.create_string_buffer(1 << 16)
    ops._lib.check(lib.skf_profiler_report(buf, len(buf)), "skf_profiler_report")
    lib.skf_profiler_enable(0)
    return {r["tag"]: round(r["ms"] / r["count"] * 1e3, 2) for r in json.loads(buf.value.decode())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=128)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--line-width", type=float, default=1.5)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()

    import torch
    from sketchformer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("raster_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    B, n = args.sketches, args.points
    s3 = sketches(B, n)
    data = torch.from_numpy(s3).to(dev)
    lengths = torch.full((B,), n, dtype=torch.int32, device=dev)
    out = {"tool": "raster_bench", "sketches": B, "points": n, "line_width": args.line_width, "group": args.group,
           "repeats": args.repeats, "sizes": []}
    xy, pen, cnt, bounds = ops.sketch_points(data, "stroke3", lengths=lengths)
    pts_us, pts_all = timed(lambda: ops.sketch_points(data, "stroke3", lengths=lengths), args.group, args.repeats, args.warmup)
    out["sketch_points_us"], out["sketch_points_us_all"] = pts_us, pts_all
    for size in args.sizes:
        img = torch.empty(B, size, size, dtype=torch.float32, device=dev)

        def raster():
            return ops.rasterize(xy, pen, cnt, bounds, (size, size), args.line_width, 2.0, out=img)

        def both():
            p = ops.sketch_points(data, "stroke3", lengths=lengths)
            return ops.rasterize(p[0], p[1], p[2], p[3], (size, size), args.line_width, 2.0, out=img)

        r_us, r_all = timed(raster, args.group, args.repeats, args.warmup)
        b_us, b_all = timed(both, args.group, args.repeats, args.warmup)
        o_us, _ = timed(lambda: ops.raster_overlap(img, img), args.group, args.repeats, args.warmup)
        raster()
        prof = profiled(ops, lambda: (both(), ops.raster_overlap(img, img)), args.group)
        out["sizes"].append({
            "profiled_us_per_launch": prof,
            "H": size, "W": size, "rasterize_us": r_us, "rasterize_us_all": r_all, "points_and_rasterize_us": b_us,
            "points_and_rasterize_us_all": b_all, "overlap_us": o_us, "us_per_sketch": round(b_us / B, 3),
            "pairs_before_culling": float(B) * n * size * size,
            "pairs_per_s_before_culling": round(float(B) * n * size * size / (r_us * 1e-6), 1),
            "ink_share": round(float(img.mean().cpu()), 4)})
    if not args.no_host:
        from sketchformer_amd.experiments.sampled_reconstructions import write_grid_png
        rows = [[s3[i + k] for k in range(8)] for i in range(0, B - B % 8, 8)] or [[s for s in s3]]
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            write_grid_png(rows, os.path.join(tmp, "grid.png"))
            wall = time.perf_counter() - t0
        out["host_matplotlib_grid"] = {"sketches": sum(len(r) for r in rows), "wall_s": round(wall, 3),
                                       "ms_per_sketch": round(wall / sum(len(r) for r in rows) * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
