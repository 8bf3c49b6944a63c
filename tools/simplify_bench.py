#!/usr/bin/env python
"""What does stroke simplification cost?  One class-sized batch of --sketches synthetic raw-like drawings (about 150 integer points in
6 strokes each: a pen that turns slowly and moves 1 - 3 units a point on the 0 .. 255 grid, as a stroke-3 array) through
Ramer-Douglas-Peucker at --epsilon, three ways:

  host      the restatement of tests/simplify_reference.py (numpy float64, explicit stack) on the first --host-sketches drawings; wall
            clock, given as a rate
  kernels   ops.stroke3_simplify on data that is already on the device (three launches and the read of the kept count); HIP events
            around groups of --group calls, so that a timed window holds some ten milliseconds of work, divided by the group
  device    the same with the packed batch going up and the rows and offsets coming back; wall clock around a synchronise; and its
            three parts on their own, each between synchronises: the copy up, the call, the copy back (pageable host memory)

and the worst case of the level loop: --zigzags zigzag polylines of 257 and of SKF_RDP_LDS_POINTS + 5 points (tests/simplify_reference.py:
every level keeps one point, n - 1 levels; the longer one runs from the workspace) through ops.rdp_keep, HIP events around groups of
--zigzag-group calls, beside the host restatement of one of them.  --repeats timed runs after a warm-up, medians.  The device results are compared with the host's, bit for
bit, on the drawings the host ran.  Out goes ONE JSON line; with --record also a text record (profiles/simplify_bench.txt).  There is
no threshold: the numbers are the finding.

    python tools/simplify_bench.py --record profiles/simplify_bench.txt
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

STROKES, LONGEST = 6, 45


def make_batch(np, n, seed):
    """(flat float32 (P, 3), offsets int64 (n + 1)) of n drawings of STROKES strokes of 5 .. LONGEST points, built in one piece."""
    rng = np.random.RandomState(seed)
    S = n * STROKES
    lens = rng.randint(5, LONGEST + 1, size=S)
    heading = rng.uniform(0, 2 * np.pi, size=(S, 1)) + np.cumsum(rng.normal(0, 0.15, size=(S, LONGEST)), axis=1)
    step = rng.uniform(1, 3, size=(S, LONGEST))
    pos = np.stack([np.cumsum(step * np.cos(heading), axis=1), np.cumsum(step * np.sin(heading), axis=1)], axis=2)
    pos = np.rint(pos + rng.uniform(40, 215, size=(S, 1, 2)))
    valid = np.arange(LONGEST)[None, :] < lens[:, None]
    points = pos[valid]                                              # stroke after stroke, drawing after drawing
    per_drawing = lens.reshape(n, STROKES).sum(1)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(per_drawing, out=offsets[1:])
    flat = np.zeros((len(points), 3), np.float32)
    flat[:, :2] = points
    flat[1:, :2] -= points[:-1]
    flat[offsets[1:-1], :2] = points[offsets[1:-1]]                  # the first row of a drawing counts from (0, 0)
    flat[np.cumsum(lens) - 1, 2] = 1
    return flat, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=70000)
    ap.add_argument("--host-sketches", type=int, default=1000)
    ap.add_argument("--zigzags", type=int, default=4096)
    ap.add_argument("--epsilon", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--zigzag-group", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import simplify_reference as ref
    from sketchformer_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    flat, offsets = make_batch(np, args.sketches, args.seed)
    P, H = len(flat), min(args.host_sketches, args.sketches)
    out = {"tool": "simplify_bench", "device": torch.cuda.get_device_name(0), "sketches": args.sketches, "points": P,
           "strokes": args.sketches * STROKES, "epsilon": args.epsilon, "repeats": args.repeats, "group": args.group, "zigzag_group": args.zigzag_group,
           "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0), "lds_points": ops.RDP_LDS_POINTS}

    def events(fn, items, group):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(group):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / group)
        med = statistics.median(ms)
        return {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "per_s": round(items / (med * 1e-3), 1)}

    def wall(fn, items, repeats):
        fn()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        return res, {"s": round(med, 6), "s_all": [round(t, 6) for t in ts], "per_s": round(items / med, 1)}

    # the device, launches alone and end to end
    flat_d, off_d = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
    out["kernels"] = events(lambda: ops.stroke3_simplify(flat_d, off_d, args.epsilon), args.sketches, args.group)

    def end_to_end():
        rows, offs = ops.stroke3_simplify(torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), args.epsilon)
        res = rows.cpu().numpy(), offs.cpu().numpy()
        torch.cuda.synchronize()
        return res
    (rows, offs), out["device_end_to_end"] = wall(end_to_end, args.sketches, args.repeats)
    out["points_kept"] = int(offs[-1])

    # its three parts, each between synchronises
    def synced(fn):
        def run():
            res = fn()
            torch.cuda.synchronize()
            return res
        return run
    up_bytes = flat.nbytes + offsets.nbytes
    _, out["copy_up"] = wall(synced(lambda: (torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev))), args.sketches, args.repeats)
    (rows_d, offs_d), out["call"] = wall(synced(lambda: ops.stroke3_simplify(flat_d, off_d, args.epsilon)), args.sketches, args.repeats)
    back_bytes = rows_d.numel() * 4 + offs_d.numel() * 8
    _, out["copy_back"] = wall(synced(lambda: (rows_d.cpu().numpy(), offs_d.cpu().numpy())), args.sketches, args.repeats)
    for leg, nbytes in (("copy_up", up_bytes), ("copy_back", back_bytes)):
        out[leg]["bytes"] = int(nbytes)
        out[leg]["gb_per_s"] = round(nbytes / max(out[leg]["s"], 1e-9) / 1e9, 2)

    # the host restatement on the first H drawings
    subset = [flat[offsets[i]:offsets[i + 1]] for i in range(H)]
    want, out["host"] = wall(lambda: ref.simplify_all(subset, args.epsilon), H, min(args.repeats, 3))
    out["host"]["sketches"] = H
    got = [rows[offs[i]:offs[i + 1]] for i in range(H)]
    out["bit_equal_on_host_subset"] = bool(ref.n_differing(got, want) == 0 and all(g.shape == w.shape for g, w in zip(got, want)))
    out["kernels_over_host"] = round(out["kernels"]["per_s"] / out["host"]["per_s"], 1)
    out["end_to_end_over_host"] = round(out["device_end_to_end"]["per_s"] / out["host"]["per_s"], 1)

    # the worst case: one point a level
    out["zigzag"] = {}
    for n in (257, ops.RDP_LDS_POINTS + 5):
        line = ref.zigzag(n)
        xy_d = torch.from_numpy(np.tile(line, (args.zigzags, 1))).to(dev)
        zo_d = torch.arange(args.zigzags + 1, dtype=torch.int64, device=dev) * n
        leg = events(lambda: ops.rdp_keep(xy_d, zo_d, args.epsilon), args.zigzags, args.zigzag_group)
        keep = ops.rdp_keep(xy_d, zo_d, args.epsilon).cpu().numpy()
        (mask, depth), host = wall(lambda: ref.rdp_mask(line, args.epsilon, return_depth=True), 1, 3)
        leg.update({"points": n, "polylines": args.zigzags, "levels": int(depth), "all_kept": bool(keep.all() and mask.all()),
                    "where": "LDS" if n <= ops.RDP_LDS_POINTS else "workspace", "host_one_polyline_s": host["s"]})
        out["zigzag"][str(n)] = leg
    print(json.dumps(out))
    if args.record:
        k, d, h = out["kernels"], out["device_end_to_end"], out["host"]
        with open(args.record, "w") as f:
            f.write("tools/simplify_bench.py on %s, %d CPUs: %d synthetic raw-like drawings = %d integer points in %d strokes,\n"
                    % (out["device"], out["cpus"], args.sketches, P, out["strokes"]))
            f.write("Ramer-Douglas-Peucker at epsilon %g keeps %d points (%.1f %%); %d timed runs after a warm-up, medians, all legs in one job on one box;\n"
                    "a HIP-event window holds %d calls of skf_stroke3_simplify or %d of skf_rdp_f32 and is divided by that number.\n\n"
                    % (args.epsilon, out["points_kept"], 100.0 * out["points_kept"] / P, args.repeats, args.group, args.zigzag_group))
            f.write("drawings per second                                                     median        every run\n")
            f.write("  host restatement (numpy float64), first %6d drawings            %12.0f  (%.4f s)  %s\n" % (H, h["per_s"], h["s"], h["s_all"]))
            f.write("  skf_stroke3_simplify alone, HIP events (incl. the read of P')     %12.0f  (%.4f ms) %s\n" % (k["per_s"], k["ms"], k["ms_all"]))
            f.write("  device end to end (packed batch up, rows and offsets back)        %12.0f  (%.4f s)  %s\n" % (d["per_s"], d["s"], d["s_all"]))
            f.write("    its parts, each between synchronises (wall clock):\n")
            for leg, what in (("copy_up", "rows and offsets up"), ("call", "ops.stroke3_simplify"), ("copy_back", "kept rows and offsets back")):
                z = out[leg]
                f.write("      %-28s %.6f s  %s%s\n" % (what, z["s"], z["s_all"],
                                                        "  = %.1f MB at %.2f GB/s" % (z["bytes"] / 1e6, z["gb_per_s"]) if "bytes" in z else ""))
            f.write("\nover the host restatement: launches alone %.1f x, end to end %.1f x; bit-equal to it on the drawings it ran: %s\n"
                    % (out["kernels_over_host"], out["end_to_end_over_host"], out["bit_equal_on_host_subset"]))
            f.write("\nworst case, zigzag polylines through skf_rdp_f32 (one kept point a level), %d polylines a call, HIP events:\n" % args.zigzags)
            for n, z in out["zigzag"].items():
                f.write("  %4s points, %4d levels, from the %-9s  %10.4f ms a call  %12.0f polylines/s  all kept: %s  (host, one polyline: %.4f s)\n"
                        % (n, z["levels"], z["where"], z["ms"], z["per_s"], z["all_kept"], z["host_one_polyline_s"]))
            f.write("Not measured: the packing of a list of drawings into one array, which comes before all three legs.\n\n")
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
