#!/usr/bin/env python
"""What does arc-length resampling cost, alone and in front of the simplification?  The class-sized batch of tools/simplify_bench.py
(--sketches synthetic raw-like drawings, about 150 integer points in 6 strokes each), every stroke a polyline of absolute points,
resampled at --spacing (ops.polyline_resample) on data that is already on the device:

  launches  HIP events around groups of --group calls, so that a timed window holds milliseconds of work, divided by the group: the
            count phase (the measure launch and the offsets scan), the count phase on as many EMPTY polylines (the scan and a
            measure launch whose waves leave at once: what of the count phase is not measuring), and the emit launch alone into
            rows allocated once; the emit launch's bytes - the table, 8 B a point, read once and 8 B a row written - per second
            beside the HBM rate the box can reach
  chain     ops.polyline_resample + ops.rdp_keep on the resampled points (the read-back of the row count included) against
            ops.rdp_keep on the points as they come: what the published recipe's extra step costs a class; and how many resampled
            strokes exceed SKF_RDP_LDS_POINTS and run the simplification from its workspace
  host      the restatement of tests/resample_reference.py on the strokes of the first --host-sketches drawings, wall clock, and
            the device rows of those strokes compared with it bit for bit

--repeats timed runs after a warm-up, medians.  Out goes ONE JSON line; with --record also a text record
(profiles/resample_bench.txt).  There is no threshold: the numbers are the finding.

    python tools/resample_bench.py --record profiles/resample_bench.txt
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_ACHIEVABLE_TB_S = 6.3                 # what a float4 copy reaches on an MI355X (8.0 by the specification)


def polylines(np, flat, offsets):
    """The stroke-3 batch of simplify_bench.make_batch -> (xy float32 (P, 2) absolute, stroke offsets int64 (S + 1))."""
    run = np.cumsum(flat[:, :2].astype(np.float64), axis=0)
    start = np.concatenate([np.zeros((1, 2)), run])[offsets[:-1]]
    xy = (run - np.repeat(start, np.diff(offsets), axis=0)).astype(np.float32)
    ends = np.flatnonzero(flat[:, 2] == 1) + 1
    return np.ascontiguousarray(xy), np.concatenate([[0], ends]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=70000)
    ap.add_argument("--host-sketches", type=int, default=1000)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--epsilon", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import resample_reference as rr
    from simplify_bench import STROKES, make_batch
    from sketchformer_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    xy, offsets = polylines(np, *make_batch(np, args.sketches, args.seed))
    P, S, H = len(xy), len(offsets) - 1, min(args.host_sketches, args.sketches)
    out = {"tool": "resample_bench", "device": torch.cuda.get_device_name(0), "sketches": args.sketches, "strokes": S, "points": P,
           "spacing": args.spacing, "epsilon": args.epsilon, "repeats": args.repeats, "group": args.group,
           "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0), "lds_points": ops.RDP_LDS_POINTS}

    def events(fn, group):
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
        return {"ms": round(statistics.median(ms), 4), "ms_all": [round(x, 4) for x in ms]}

    def wall(fn, repeats):
        fn()
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return res, {"s": round(statistics.median(ts), 6), "s_all": [round(t, 6) for t in ts]}

    xy_d, off_d = torch.from_numpy(xy).to(dev), torch.from_numpy(offsets).to(dev)
    out_offsets, ws, nbytes = ops.polyline_resample_offsets(xy_d, off_d, args.spacing, return_workspace=True)
    rows = int(out_offsets[-1].item())
    out["rows"] = rows
    out_xy = torch.empty(rows, 2, dtype=torch.float32, device=dev)
    per_stroke = np.diff(out_offsets.cpu().numpy())
    out["longest_stroke_rows"] = int(per_stroke.max())
    out["strokes_above_lds_points"] = int((per_stroke > ops.RDP_LDS_POINTS).sum())

    # the launches
    stream = ops._stream
    p = ops._p
    empty_offsets = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    scratch_offsets = torch.empty(S + 1, dtype=torch.int64, device=dev)
    out["count_phase"] = events(lambda: _lib.call("skf_polyline_resample_count", p(xy_d), 2, P, p(off_d), S, args.spacing, p(scratch_offsets),
                                                  p(ws), nbytes, stream()), args.group)
    assert torch.equal(scratch_offsets, out_offsets)
    idle_ws = torch.empty_like(ws)
    out["count_phase_on_empty_polylines"] = events(lambda: _lib.call("skf_polyline_resample_count", p(xy_d), 2, P, p(empty_offsets), S,
                                                                    args.spacing, p(scratch_offsets), p(idle_ws), nbytes, stream()), args.group)
    out["emit"] = events(lambda: _lib.call("skf_polyline_resample_emit", p(xy_d), 2, P, p(off_d), S, args.spacing, p(out_offsets), p(out_xy),
                                           rows, p(ws), nbytes, stream()), args.group)
    emit_bytes = 8 * P + 8 * rows
    out["emit"]["bytes"] = emit_bytes
    out["emit"]["tb_per_s"] = round(emit_bytes / (out["emit"]["ms"] * 1e-3) / 1e12, 3)
    out["emit"]["rows_per_s"] = round(rows / (out["emit"]["ms"] * 1e-3), 1)
    out["hbm_achievable_tb_per_s"] = HBM_ACHIEVABLE_TB_S

    # the chain against the simplification alone
    def chain():
        r_xy, r_off = ops.polyline_resample(xy_d, off_d, args.spacing)
        return r_xy, r_off, ops.rdp_keep(r_xy, r_off, args.epsilon)
    out["rdp_alone"] = events(lambda: ops.rdp_keep(xy_d, off_d, args.epsilon), args.group)
    out["resample_then_rdp"] = events(chain, args.group)
    r_xy, r_off, keep = chain()
    out["kept_after_resampling"] = int(keep.sum().item())
    out["kept_without"] = int(ops.rdp_keep(xy_d, off_d, args.epsilon).sum().item())
    out["rdp_on_resampled_alone"] = events(lambda: ops.rdp_keep(r_xy, r_off, args.epsilon), args.group)

    # the host restatement on the strokes of the first H drawings
    n_host = H * STROKES
    subset = [xy[offsets[i]:offsets[i + 1]] for i in range(n_host)]
    want, out["host"] = wall(lambda: rr.resample_all(subset, args.spacing), min(args.repeats, 3))
    out["host"].update({"sketches": H, "strokes": n_host, "rows": int(sum(len(w) for w in want))})
    got_xy, got_off = r_xy.cpu().numpy(), r_off.cpu().numpy()
    want_xy, want_off = rr.pack(want)
    out["bit_equal_on_host_subset"] = bool(np.array_equal(got_off[:n_host + 1], want_off) and rr.same_bits(got_xy[:want_off[-1]], want_xy))
    device_rows_per_s = rows / ((out["count_phase"]["ms"] + out["emit"]["ms"]) * 1e-3)
    out["launches_over_host"] = round(device_rows_per_s / (out["host"]["rows"] / out["host"]["s"]), 1)
    print(json.dumps(out))
    if args.record:
        c, z, e, h = out["count_phase"], out["count_phase_on_empty_polylines"], out["emit"], out["host"]
        with open(args.record, "w") as f:
            f.write("tools/resample_bench.py on %s, %d CPUs: the %d synthetic raw-like drawings of tools/simplify_bench.py = %d integer points in\n"
                    "%d strokes, every stroke resampled along its arc length at a spacing of %g: %d rows (%.2f x the points), at most %d on one\n"
                    "stroke; %d timed runs after a warm-up, medians, all legs in one job on one box; a HIP-event window holds %d calls and is\n"
                    "divided by that number.\n\n"
                    % (out["device"], out["cpus"], args.sketches, P, S, args.spacing, rows, rows / P, out["longest_stroke_rows"], args.repeats, args.group))
            f.write("the launches, data on the device                                          median ms   every run\n")
            f.write("  count phase: measure launch + offsets scan                              %9.4f   %s\n" % (c["ms"], c["ms_all"]))
            f.write("  the same on %7d empty polylines (scan + a measure launch that idles)  %9.4f   %s\n" % (S, z["ms"], z["ms_all"]))
            f.write("  emit launch alone                                                       %9.4f   %s\n" % (e["ms"], e["ms_all"]))
            f.write("    = %.0f rows/s; %.1f MB (8 B a point of the table + 8 B a row written) at %.3f TB/s, beside the %.1f TB/s a copy reaches in HBM:\n"
                    "    %.1f %% of it.  The emit launch is not a stream: every lane walks a binary search over its stroke's table (cache hits)\n"
                    "    and divides in fp64 before its one 8-byte store.\n"
                    % (e["rows_per_s"], emit_bytes / 1e6, e["tb_per_s"], HBM_ACHIEVABLE_TB_S, 100.0 * e["tb_per_s"] / HBM_ACHIEVABLE_TB_S))
            f.write("\nthe chain, data on the device (ops level, allocations and the 8-byte read-back of the row count included)\n")
            f.write("  ops.rdp_keep on the points as they come (today's recipe)                %9.4f   %s\n" % (out["rdp_alone"]["ms"], out["rdp_alone"]["ms_all"]))
            f.write("  ops.polyline_resample + ops.rdp_keep on its rows (the published steps)  %9.4f   %s\n"
                    % (out["resample_then_rdp"]["ms"], out["resample_then_rdp"]["ms_all"]))
            f.write("    of which ops.rdp_keep on the resampled rows                           %9.4f   %s\n"
                    % (out["rdp_on_resampled_alone"]["ms"], out["rdp_on_resampled_alone"]["ms_all"]))
            f.write("  kept at epsilon %g: %d points without the step, %d with it; resampled strokes above SKF_RDP_LDS_POINTS = %d (workspace path): %d\n"
                    % (args.epsilon, out["kept_without"], out["kept_after_resampling"], ops.RDP_LDS_POINTS, out["strokes_above_lds_points"]))
            f.write("\nhost restatement (numpy), the %d strokes of the first %d drawings = %d rows: %.4f s  %s\n"
                    % (n_host, H, h["rows"], h["s"], h["s_all"]))
            f.write("  rows per second, count phase + emit launch over the host: %.1f x; bit-equal to it on those strokes: %s\n"
                    % (out["launches_over_host"], out["bit_equal_on_host_subset"]))
            f.write("Not measured: the packing of a list of drawings into one array and the copies between host and device.\n\n")
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
