#!/usr/bin/env python
"""Times the shape-distance kernel (ops.shape_distance over skf_chamfer.hip) at the sizes a user runs: paired, B = 128 pairs of
L = 200 (a validation batch against its reconstructions), and cross, 256 queries x 4096 gallery rows (the distance matrix of a
retrieval baseline) with every sketch full-length and with QuickDraw-like lengths (synthetic.continuous_batch, the generator of
the other bench tools) - against two yardsticks on the same inputs on the same machine:

  host      the float32 restatement of tests/shape_reference.py: all pairs of the paired case, a few entries of each matrix.  The
            device results of those pairs must be equal to it BIT FOR BIT (asserted before anything is timed).
  compose   a torch composition on the device: the broadcast (samples x primitives) table of point-segment distances, reduced with
            amin, built for all queries against a slab of --slab gallery rows at a time (what fits).  Its means are plain float32
            means, so it is compared with a tolerance (asserted), not bit for bit.

Device times are HIP events around groups of calls after a warm-up, the median over --repeats, divided by the group size.  An
evaluation is one (sample, primitive) pair of the rule: a dot or a segment of one sketch against a sample of the other, both
directions counted; evaluations per second = that count / time.  Out goes ONE JSON line; with --record also a text record
(profiles/chamfer_bench.txt).

    python tools/chamfer_bench.py
    python tools/chamfer_bench.py --pairs 128 --length 200 --queries 256 --gallery 4096 --samples 4 --record profiles/chamfer_bench.txt
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


def composition(S):
    """-> fn(xa, pa, na, xb, pb, nb, cross) -> (Q, G, 4) or (B, 4) float32: the rule as eager torch on padded tensors"""
    import torch

    def prepared(xy, pen, n):
        N, T, _ = xy.shape
        idx = torch.arange(T, device=xy.device)[None, :]
        L = n.clamp(min=1)[:, None]                                # an empty sketch: the point (0, 0)
        xy = torch.where((idx < n[:, None])[:, :, None], xy, torch.zeros_like(xy))
        prev = torch.roll(xy, 1, dims=1)
        seg = (idx > 0) & (idx < n[:, None]) & (torch.roll(pen, 1, dims=1) == 0)
        a = torch.where(seg[:, :, None], prev, xy)                 # no segment: a = p, e = 0 - the dot once more
        e = xy - a
        len2 = e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]
        inv = torch.where(len2 > 0, 1.0 / len2, torch.zeros_like(len2))
        t = (torch.arange(S, device=xy.device, dtype=torch.float32) / float(S))[None, None, :, None]
        smp = torch.where((t > 0), a[:, :, None, :] + t * e[:, :, None, :], xy[:, :, None, :]).reshape(N, T * S, 2)
        ok = ((idx < L)[:, :, None] & ((t[:, :, :, 0] == 0) | seg[:, :, None])).reshape(N, T * S)
        return dict(p=xy, a=a, e=e, inv=inv, live=idx < L, smp=smp, ok=ok)

    def directed(X, Y, cross):                                     # samples of X (Q, M) against primitives of Y (G, T) -> mean, max
        if cross:                                                  # the table is (Q, G, M, T) ...
            sx, sy, ok = X["smp"][:, None, :, None, 0], X["smp"][:, None, :, None, 1], X["ok"][:, None, :]
            cut = lambda v: v[None, :, None, :]                    # noqa: E731
        else:                                                      # ... or (B, M, T) for the pairs
            sx, sy, ok = X["smp"][:, :, None, 0], X["smp"][:, :, None, 1], X["ok"]
            cut = lambda v: v[:, None, :]                          # noqa: E731
        qx, qy = sx - cut(Y["p"][:, :, 0]), sy - cut(Y["p"][:, :, 1])
        d2 = qx * qx + qy * qy
        px, py = sx - cut(Y["a"][:, :, 0]), sy - cut(Y["a"][:, :, 1])
        ex, ey = cut(Y["e"][:, :, 0]), cut(Y["e"][:, :, 1])
        t = ((px * ex + py * ey) * cut(Y["inv"])).clamp(0.0, 1.0)
        rx, ry = px - t * ex, py - t * ey
        d2 = torch.minimum(d2, rx * rx + ry * ry)
        d2 = torch.where(cut(Y["live"]), d2, torch.full_like(d2, float("inf")))
        d = torch.amin(d2, dim=-1).sqrt()                          # (Q, G, M) or (B, M)
        d = torch.where(ok, d, torch.zeros_like(d))
        count = X["ok"].sum(dim=1)
        return d.sum(dim=-1) / (count[:, None] if cross else count), d.amax(dim=-1)

    def fn(xa, pa, na, xb, pb, nb, cross):
        A, B = prepared(xa, pa, na), prepared(xb, pb, nb)
        mab, xab = directed(A, B, cross)
        mba, xba = directed(B, A, cross)                           # (cross: as (G, Q), transposed below)
        if cross:
            mba, xba = mba.t(), xba.t()
        return torch.stack([mab, mba, xab, xba], dim=-1)
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--gallery", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--slab", type=int, default=4, help="gallery rows per slab of the torch composition")
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--cross-group", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--entries", type=int, default=12, help="entries of each matrix the host restatement checks")
    ap.add_argument("--no-compose", action="store_true")
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import shape_reference as ref
    from sketchformer_amd import ops, raster, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_bench needs the GPU: nothing here is measured on the host alone")
    B, L, Q, G, S = args.pairs, args.length, args.queries, args.gallery, args.samples
    out = {"pairs": B, "length": L, "queries": Q, "gallery": G, "samples_per_segment": S, "device": torch.cuda.get_device_name(0)}

    def sketches(n, seed, full):                                   # stroke-5 rows of the synthetic generator -> device points
        x, _ = synthetic.continuous_batch(n, seq_len=L, seed=seed, full=full)
        xy, pen, cnt, _ = raster.points(x, kind="stroke5")
        return xy, pen, cnt

    def host(t, i):
        xy, pen, n = (v.cpu().numpy() for v in t)
        return xy[i, :n[i]], pen[i, :n[i]]

    def evaluations(ta, tb, cross):                                # (samples of a) x (dots + segments of b), both ways, summed over the pairs
        def counts(t):
            _, pen, n = t
            idx = torch.arange(pen.shape[1], device=pen.device)[None, :]
            segs = ((idx > 0) & (idx < n[:, None]) & (torch.roll(pen, 1, dims=1) == 0)).sum(dim=1).double()
            pts = n.clamp(min=1).double()
            return pts + (S - 1) * segs, pts + segs                # samples, primitives
        (sa, pa), (sb, pb) = counts(ta), counts(tb)
        if cross:
            return float(sa.sum() * pb.sum() + sb.sum() * pa.sum())
        return float((sa * pb + sb * pa).sum())

    cases = {
        "paired_full": (sketches(B, 1, True), sketches(B, 2, True), False, args.group),
        "cross_full": (sketches(Q, 3, True), sketches(G, 4, True), True, args.cross_group),
        "cross_ragged": (sketches(Q, 5, False), sketches(G, 6, False), True, args.cross_group),
    }
    compose = composition(S)
    host_s = None
    for name, (ta, tb, cross, group) in cases.items():
        fn = lambda ta=ta, tb=tb, cross=cross: ops.shape_distance(*ta, *tb, samples_per_segment=S, cross=cross)      # noqa: E731
        got = fn().cpu().numpy()
        # the timed inputs give the restatement's results, bit for bit
        if cross:
            rng = np.random.RandomState(7)
            picks = [(0, 0), (len(ta[0]) - 1, len(tb[0]) - 1)] + [(int(rng.randint(len(ta[0]))), int(rng.randint(len(tb[0])))) for _ in range(args.entries - 2)]
            for i, j in picks:
                assert got[i, j].tobytes() == ref.shape_ref(*host(ta, i), *host(tb, j), S).tobytes(), (name, i, j)
            checked = "%d entries equal to the host restatement bit for bit" % len(picks)
        else:
            t0 = time.perf_counter()
            want = np.array([ref.shape_ref(*host(ta, i), *host(tb, i), S) for i in range(len(ta[0]))], np.float32)
            host_s = time.perf_counter() - t0
            assert got.tobytes() == want.tobytes(), name
            checked = "all %d pairs equal to the host restatement bit for bit" % len(want)
        us, all_us = timed(fn, group, args.repeats, args.warmup)
        ev = evaluations(ta, tb, cross)
        r = {"us": us, "repeats_us": all_us, "pairs": len(ta[0]) * (len(tb[0]) if cross else 1), "evaluations": ev,
             "evaluations_per_s": round(ev / (us * 1e-6), 1), "mean_points": round(float(tb[2].double().mean()), 1),
             "checked": checked}
        if not cross:
            r["host_s"] = round(host_s, 4)
            r["host_evaluations_per_s"] = round(ev / host_s, 1)
            r["host_over_device"] = round(host_s / (us * 1e-6), 1)
        if not args.no_compose:
            def composed(ta=ta, tb=tb, cross=cross):
                if not cross:                                      # the pairs: one (B, samples, primitives) table
                    return compose(*ta, *tb, False)
                return torch.cat([compose(*ta, *(v[at:at + args.slab] for v in tb), True) for at in range(0, len(tb[0]), args.slab)], dim=1)
            compose(*(v[:2] for v in ta), *(v[:2] for v in tb), cross)                       # warm-up: two rows a side
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            other = composed()
            torch.cuda.synchronize()
            compose_s = time.perf_counter() - t0
            other = other.cpu().numpy()
            # maxima: the same expressions, a square root that may differ in its last bit; means: float32 sums of ~800 terms
            err = float(np.abs(other - got).max() / max(float(np.abs(got).max()), 1e-30))
            assert err <= 1e-5, (name, err)
            r.update(compose_s=round(compose_s, 4), compose_over_device=round(compose_s / (us * 1e-6), 1),
                     compose_evaluations_per_s=round(ev / compose_s, 1), compose_max_rel_diff=err)
        out[name] = r
    print(json.dumps(out))
    if args.record:
        with open(args.record, "w") as f:
            f.write("tools/chamfer_bench.py on %s: HIP events, median of %d repeats (groups of %d paired / %d cross calls, %d warm-up calls), "
                    "samples_per_segment = %d\n\n" % (out["device"], args.repeats, args.group, args.cross_group, args.warmup, S))
            f.write("%-13s %9s %8s %14s %12s %10s   %s\n" % ("case", "pairs", "points", "evaluations", "time (us)", "Geval/s", "repeats (us)"))
            for name in cases:
                r = out[name]
                f.write("%-13s %9d %8.1f %14.4g %12.2f %10.2f   %s\n" % (name, r["pairs"], r["mean_points"], r["evaluations"], r["us"],
                                                                      r["evaluations_per_s"] / 1e9, r["repeats_us"]))
            f.write("\npaired_full = %d pairs of L = %d; cross_full = %d x %d rows of L = %d; cross_ragged = the same matrix with QuickDraw-like "
                    "lengths (synthetic.continuous_batch); points = mean points per gallery sketch\n" % (B, L, Q, G, L))
            f.write("an evaluation is one (sample, dot or segment) pair of the rule, both directions counted\n\n")
            for name in cases:
                r = out[name]
                f.write("%-13s %s\n" % (name, r["checked"]))
                if "host_s" in r:
                    f.write("%-13s host restatement (tests/shape_reference.py), the same pairs, wall clock: %.3f s = %.3g Geval/s (%.0f x the device call)\n"
                            % ("", r["host_s"], r["host_evaluations_per_s"] / 1e9, r["host_over_device"]))
                if "compose_s" in r:
                    f.write("%-13s torch composition on the device (%s), wall clock of one run after a warm-up: %.4f s = %.3g Geval/s (%.1f x the "
                            "kernel's time; largest relative difference to the kernel %.2g)\n"
                            % ("", "one table for all pairs" if name.startswith("paired") else "slabs of %d gallery rows" % args.slab, r["compose_s"],
                               r["compose_evaluations_per_s"] / 1e9, r["compose_over_device"], r["compose_max_rel_diff"]))
            build = os.path.join(ROOT, "profiles", "chamfer_build.txt")
            if os.path.exists(build):                              # registers and LDS of the kernel as compiled
                with open(build) as b:
                    f.write("\n" + b.read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
