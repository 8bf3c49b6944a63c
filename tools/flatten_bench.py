#!/usr/bin/env python
"""What does flattening SVG-like paths cost, alone and as the first step of svg.svg_to_stroke3?  A class-sized batch (--drawings
synthetic drawings of 6 subpaths x 8 connected cubics each, seeded, in the working frame of sketchformer_amd/svg.py: larger side
1024) flattened at --tol (ops.path_flatten) on data that is already on the device:

  launches  HIP events around groups of --group calls, divided by the group: the count phase (the count launch and the offsets
            scan) and the emit launch alone into rows allocated once; the emit launch's rows per second and its bytes - 64 B of
            control points and 8 B of running sum a segment read, 8 B a row written - per second, beside a device-to-device copy of
            as many bytes as the emit launch writes, timed in the same run (the copy reads and writes: twice those bytes move)
  chain     svg.svg_to_stroke3 on the parsed drawings (parsing is not part of it: the drawings are built as control points),
            wall clock: working frame and packing on the host, flatten, normalise, RDP, kept rows back, stroke-3 on the host
  host      the restatement of tests/flatten_reference.py on the subpaths of the first --host-drawings drawings, wall clock, and
            the device rows of those subpaths compared with it bit for bit

--repeats timed runs after a warm-up, medians.  Out goes ONE JSON line; with --record also a text record
(profiles/flatten_bench.txt).  There is no threshold: the numbers are the finding.

    python tools/flatten_bench.py --record profiles/flatten_bench.txt
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

SUBPATHS, CUBICS = 6, 8
FP64_OPS_PER_ROW = 36                     # 6 lerps x 3 operations x 2 coordinates; one division besides


def make_batch(np, drawings, seed):
    """-> ctrl (G, 4, 2) float64: drawings x SUBPATHS x CUBICS connected cubics, every drawing in its working frame already"""
    rng = np.random.RandomState(seed)
    S = drawings * SUBPATHS
    step = rng.normal(0.0, 25.0, size=(S, CUBICS * 3, 2))
    start = rng.uniform(200.0, 800.0, size=(S, 1, 2))
    pts = np.concatenate([start, start + np.cumsum(step, axis=1)], axis=1)            # (S, 3 CUBICS + 1, 2)
    pts = pts.reshape(drawings, -1, 2)
    lo = pts.min(axis=1, keepdims=True)
    pts = (pts - lo) * (1024.0 / (pts.max(axis=1, keepdims=True) - lo).max(axis=2, keepdims=True))
    pts = pts.reshape(S, 3 * CUBICS + 1, 2)
    idx = (3 * np.arange(CUBICS))[:, None] + np.arange(4)[None, :]
    return np.ascontiguousarray(pts[:, idx].reshape(S * CUBICS, 4, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drawings", type=int, default=70000)
    ap.add_argument("--host-drawings", type=int, default=1000)
    ap.add_argument("--tol", type=float, default=0.0625)
    ap.add_argument("--epsilon", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import flatten_reference as fr
    from sketchformer_amd import _lib, ops, svg
    if not torch.cuda.is_available():
        raise SystemExit("flatten_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    ctrl = make_batch(np, args.drawings, args.seed)
    G, S, H = len(ctrl), args.drawings * SUBPATHS, min(args.host_drawings, args.drawings)
    kind = np.ones(G, np.int32)
    offsets = np.arange(S + 1, dtype=np.int64) * CUBICS
    out = {"tool": "flatten_bench", "device": torch.cuda.get_device_name(0), "drawings": args.drawings, "subpaths": S, "segments": G,
           "tol": args.tol, "epsilon": args.epsilon, "repeats": args.repeats, "group": args.group,
           "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}

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
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = fn()
            ts.append(time.perf_counter() - t0)
        return res, {"s": round(statistics.median(ts), 6), "s_all": [round(t, 6) for t in ts]}

    ctrl_d, kind_d, off_d = torch.from_numpy(ctrl).to(dev), torch.from_numpy(kind).to(dev), torch.from_numpy(offsets).to(dev)
    out_offsets, ws, nbytes = ops.path_flatten_offsets(ctrl_d, kind_d, off_d, args.tol, return_workspace=True)
    rows = int(out_offsets[-1].item())
    pieces = fr.pieces(ctrl[:H * SUBPATHS * CUBICS], kind[:H * SUBPATHS * CUBICS], args.tol)
    out.update({"rows": rows, "pieces_min": int(pieces.min()), "pieces_max": int(pieces.max())})
    out_xy = torch.empty(rows, 2, dtype=torch.float32, device=dev)

    # the launches
    stream, p = ops._stream, ops._p
    scratch_offsets = torch.empty(S + 1, dtype=torch.int64, device=dev)
    out["count_phase"] = events(lambda: _lib.call("skf_path_flatten_count", p(ctrl_d), p(kind_d), G, p(off_d), S, args.tol, p(scratch_offsets),
                                                  p(ws), nbytes, stream()), args.group)
    assert torch.equal(scratch_offsets, out_offsets)
    out["emit"] = events(lambda: _lib.call("skf_path_flatten_emit", p(ctrl_d), p(kind_d), G, p(off_d), S, args.tol, p(out_offsets), p(out_xy),
                                           rows, p(ws), nbytes, stream()), args.group)
    e = out["emit"]
    e["bytes_read"], e["bytes_written"] = 72 * G, 8 * rows
    e["rows_per_s"] = round(rows / (e["ms"] * 1e-3), 1)
    e["written_tb_per_s"] = round(8 * rows / (e["ms"] * 1e-3) / 1e12, 4)
    e["moved_tb_per_s"] = round((72 * G + 8 * rows) / (e["ms"] * 1e-3) / 1e12, 4)
    e["fp64_tflops"] = round(FP64_OPS_PER_ROW * rows / (e["ms"] * 1e-3) / 1e12, 3)
    copy_dst = torch.empty_like(out_xy)
    out["copy_of_the_rows"] = events(lambda: copy_dst.copy_(out_xy), args.group)
    out["copy_of_the_rows"]["written_tb_per_s"] = round(8 * rows / (out["copy_of_the_rows"]["ms"] * 1e-3) / 1e12, 4)
    got_xy, got_off = out_xy.cpu().numpy(), out_offsets.cpu().numpy()
    del copy_dst, out_xy

    # the host restatement on the subpaths of the first H drawings
    n_host = H * SUBPATHS
    want, out["host"] = wall(lambda: fr.flatten(ctrl[:n_host * CUBICS], kind[:n_host * CUBICS], offsets[:n_host + 1], args.tol), min(args.repeats, 3))
    out["host"].update({"drawings": H, "subpaths": n_host, "rows": int(sum(len(w) for w in want))})
    want_xy, want_off = fr.pack(want)
    out["bit_equal_on_host_subset"] = bool(np.array_equal(got_off[:n_host + 1], want_off) and fr.same_bits(got_xy[:want_off[-1]], want_xy))
    device_rows_per_s = rows / ((out["count_phase"]["ms"] + e["ms"]) * 1e-3)
    out["launches_over_host"] = round(device_rows_per_s / (out["host"]["rows"] / out["host"]["s"]), 1)
    del got_xy

    # the chain: parsed drawings in, stroke-3 out
    drawings = [[(ctrl[(d * SUBPATHS + s) * CUBICS:(d * SUBPATHS + s + 1) * CUBICS], kind[:CUBICS]) for s in range(SUBPATHS)]
                for d in range(args.drawings)]
    svg.svg_to_stroke3(drawings[:64], epsilon=args.epsilon, tol=args.tol)          # warm-up
    sketches, out["svg_to_stroke3"] = wall(lambda: svg.svg_to_stroke3(drawings, epsilon=args.epsilon, tol=args.tol), min(args.repeats, 3))
    c = out["svg_to_stroke3"]
    c["drawings_per_s"] = round(args.drawings / c["s"], 1)
    c["kept_rows"] = int(sum(len(s) for s in sketches)) + args.drawings
    print(json.dumps(out))
    if args.record:
        k, h, cp = out["count_phase"], out["host"], out["copy_of_the_rows"]
        with open(args.record, "w") as f:
            f.write("tools/flatten_bench.py on %s, %d CPUs: %d seeded synthetic drawings of %d subpaths x %d connected cubics = %d segments, every\n"
                    "drawing in its working frame (larger side 1024), flattened at tol %g: %d rows (%.1f a segment; n from %d to %d on the host subset);\n"
                    "%d timed runs after a warm-up, medians, all legs in one job on one box; a HIP-event window holds %d calls and is divided by\n"
                    "that number.\n\n"
                    % (out["device"], out["cpus"], args.drawings, SUBPATHS, CUBICS, G, args.tol, rows, rows / G, out["pieces_min"], out["pieces_max"],
                       args.repeats, args.group))
            f.write("the launches, data on the device                                          median ms   every run\n")
            f.write("  count phase: count launch + offsets scan                                %9.4f   %s\n" % (k["ms"], k["ms_all"]))
            f.write("  emit launch alone                                                       %9.4f   %s\n" % (e["ms"], e["ms_all"]))
            f.write("  device-to-device copy of the emitted rows (%.1f MB)                    %9.4f   %s\n" % (8 * rows / 1e6, cp["ms"], cp["ms_all"]))
            f.write("    emit = %.3g rows/s: %.1f MB written at %.3f TB/s (%.1f MB moved with the reads, %.3f TB/s); the copy writes the same\n"
                    "    bytes at %.3f TB/s: the emit launch stores at %.1f %% of the copy's rate.  Its %d fp64 operations a row come to %.2f TFLOP/s.\n"
                    % (e["rows_per_s"], 8 * rows / 1e6, e["written_tb_per_s"], (72 * G + 8 * rows) / 1e6, e["moved_tb_per_s"], cp["written_tb_per_s"],
                       100.0 * e["written_tb_per_s"] / cp["written_tb_per_s"], FP64_OPS_PER_ROW, e["fp64_tflops"]))
            f.write("    Is the emit launch store-bound, as 36 fp64 operations for every 8-byte row suggested?\n    %s\n"
                    % ("It is: it writes at more than two thirds of what a plain copy of the same rows reaches."
                       if e["written_tb_per_s"] >= 0.67 * cp["written_tb_per_s"] else
                       "It is not: a plain copy stores the same rows %.1f times as fast.  What the launch waits for instead - the search\n"
                       "    through memory, the fp64 division or the lerps in front of every 8-byte store - was not measured."
                       % (cp["written_tb_per_s"] / e["written_tb_per_s"])))
            f.write("\nthe chain, wall clock: svg.svg_to_stroke3 on the %d drawings as parsed control points (no parsing): working frame and packing\n"
                    "on the host, copies, flatten, normalise, RDP at epsilon %g, the kept rows back, stroke-3 on the host\n"
                    "  %.3f s  %s  = %.0f drawings/s; %d rows kept of %d\n" % (args.drawings, args.epsilon, c["s"], c["s_all"], c["drawings_per_s"], c["kept_rows"], rows))
            f.write("\nhost restatement (numpy), the %d subpaths of the first %d drawings = %d rows: %.4f s  %s\n"
                    % (n_host, H, h["rows"], h["s"], h["s_all"]))
            f.write("  rows per second, count phase + emit launch over the host: %.1f x; bit-equal to it on those subpaths: %s\n"
                    % (out["launches_over_host"], out["bit_equal_on_host_subset"]))
            f.write("Not measured: parsing SVG text, which is host Python.\n\n")
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
