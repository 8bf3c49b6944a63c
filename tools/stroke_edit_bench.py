#!/usr/bin/env python
"""What do stroke edits cost?  The class-sized batch of tools/simplify_bench.py and tools/resample_bench.py (--sketches synthetic
raw-like drawings, about 150 integer points in 6 strokes each) on data that is already on the device:

  table     skf_stroke_table: the count launch, the offsets scan and the write launch (one lane's sequential walk per sketch);
            ops.stroke3_simplify on the same batch beside it for scale, whose mark launch holds the same walk
  permute   one random permutation of every sketch's strokes (strokes.permutation_lists): the count phase (count launch + offsets
            scan), the emit launch alone into rows allocated once, and ops.stroke_edit end to end with the table given (its
            allocations and the 8-byte read-back of the row count included)
  leave-one-out   every sketch without its stroke j, for every j (strokes.leave_one_out_lists): the same three figures; the batch
            grows by the stroke count less one
  emit      in GB/s - every output row is 12 bytes read and 12 bytes written, plus 16 bytes an entry of the workspace - beside
            the rate of a device-to-device copy measured in the same run
  host      the restatement of tests/strokes_reference.py on the first --host-sketches drawings, wall clock, and the device rows
            of those drawings compared with it bit for bit

HIP events around groups of --group calls; --repeats timed runs after a warm-up, medians.  Out goes ONE JSON line; with --record
also a text record (profiles/stroke_edit_bench.txt).  There is no threshold: the numbers are the finding.

    python tools/stroke_edit_bench.py --record profiles/stroke_edit_bench.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=70000)
    ap.add_argument("--host-sketches", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--copy-mib", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import strokes_reference as st
    from simplify_bench import make_batch
    from sketchformer_amd import _lib, ops, strokes
    if not torch.cuda.is_available():
        raise SystemExit("stroke_edit_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    flat, offsets = make_batch(np, args.sketches, args.seed)
    P, N, H = len(flat), args.sketches, min(args.host_sketches, args.sketches)
    out = {"tool": "stroke_edit_bench", "device": torch.cuda.get_device_name(0), "sketches": N, "points": P, "repeats": args.repeats,
           "group": args.group, "cpus": int(os.environ.get("OMP_NUM_THREADS", "0") or 0)}

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

    p, stream = ops._p, ops._stream
    flat_d, off_d = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)

    # the copy rate of this box, now
    words = args.copy_mib * (1 << 20) // 4
    a, b = torch.empty(words, dtype=torch.float32, device=dev), torch.zeros(words, dtype=torch.float32, device=dev)
    out["copy"] = events(lambda: a.copy_(b), args.group)
    out["copy"]["gb_per_s"] = round(2 * 4 * words / (out["copy"]["ms"] * 1e-3) / 1e9, 1)
    del a, b

    # the table
    ss = torch.empty(N + 1, dtype=torch.int64, device=dev)
    sr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    se = torch.empty(P, 4, dtype=torch.float32, device=dev)
    tws, tbytes = ops._workspace_for("skf_stroke_table_workspace_bytes", dev, P, N)
    out["table"] = events(lambda: _lib.call("skf_stroke_table", p(flat_d), P, p(off_d), N, 0, p(ss), p(sr), p(se), p(tws), tbytes, stream()),
                          args.group)
    out["table_end_to_end"] = events(lambda: ops.stroke_table(flat_d, off_d), args.group)
    out["simplify_for_scale"] = events(lambda: ops.stroke3_simplify(flat_d, off_d, 2.0), args.group)
    table = ops.stroke_table(flat_d, off_d)
    T = table[1].shape[0] - 1
    counts = np.diff(table[0].cpu().numpy())
    out["strokes"] = T

    def edit_legs(name, src, lists):
        sel, sel_offsets = strokes.pack_selections(lists)
        M, Q = len(src), len(sel)
        src_d, so_d, sel_d = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (src.astype(np.int32), sel_offsets, sel))
        oo = torch.empty(M + 1, dtype=torch.int64, device=dev)
        ws, nbytes = ops._workspace_for("skf_stroke_edit_workspace_bytes", dev, P, N, M, Q)
        count = lambda: _lib.call("skf_stroke_edit_count", P, p(table[0]), N, p(table[1]), T, p(src_d), p(so_d), M, p(sel_d), Q, 0, p(oo),
                                  p(ws), nbytes, stream())                       # noqa: E731
        leg = {"outputs": M, "entries": Q, "count_phase": events(count, args.group)}
        rows = int(oo[-1].item())
        rows_d = torch.empty(rows, 3, dtype=torch.float32, device=dev)
        emit = lambda: _lib.call("skf_stroke_edit_emit", p(flat_d), P, p(table[0]), N, p(table[1]), p(table[2]), T, p(src_d), p(so_d), M,
                                 p(sel_d), Q, 0, p(oo), p(rows_d), rows, p(ws), nbytes, stream())      # noqa: E731
        leg["emit"] = events(emit, args.group)
        leg["rows"] = rows
        leg["emit"]["bytes"] = 24 * rows + 16 * Q
        leg["emit"]["gb_per_s"] = round(leg["emit"]["bytes"] / (leg["emit"]["ms"] * 1e-3) / 1e9, 1)
        del rows_d
        leg["end_to_end"] = events(lambda: ops.stroke_edit(flat_d, off_d, src_d, so_d, sel_d, table=table), max(args.group // 2, 1))
        got = ops.stroke_edit(flat_d, off_d, src_d, so_d, sel_d, table=table)
        out[name] = leg
        return got

    perm_lists = strokes.permutation_lists(counts, seed=args.seed)
    got_perm = edit_legs("permute", np.arange(N), perm_lists)
    loo_lists, owner, _ = strokes.leave_one_out_lists(counts)
    got_loo = edit_legs("leave_one_out", owner, loo_lists)

    # the host restatement on the first H drawings
    sketches = [flat[offsets[i]:offsets[i + 1]] for i in range(H)]
    n_loo = int(np.searchsorted(owner, H))

    def host():
        return st.edit(sketches, range(H), perm_lists[:H]), st.edit(sketches, owner[:n_loo], loo_lists[:n_loo])
    t0 = time.perf_counter()
    want_perm, want_loo = host()
    out["host"] = {"s": round(time.perf_counter() - t0, 4), "sketches": H, "rows": int(sum(len(w) for w in want_perm + want_loo))}
    ok = True
    for got, want in ((got_perm, want_perm), (got_loo, want_loo)):
        want_flat, want_off = st.pack(want)
        ok = ok and np.array_equal(got[1][:len(want) + 1].cpu().numpy(), want_off) \
            and st.same_bits(got[0][:len(want_flat)].cpu().numpy(), want_flat)
    out["bit_equal_on_host_subset"] = bool(ok)
    dev_rows = out["permute"]["rows"] + out["leave_one_out"]["rows"]
    dev_s = sum(out[k][leg]["ms"] for k in ("permute", "leave_one_out") for leg in ("count_phase", "emit")) * 1e-3
    out["launches_over_host"] = round((dev_rows / dev_s) / (out["host"]["rows"] / out["host"]["s"]), 1)
    print(json.dumps(out))
    if args.record:
        with open(args.record, "w") as f:
            f.write("tools/stroke_edit_bench.py on %s, %d CPUs: the %d synthetic raw-like drawings of tools/simplify_bench.py = %d integer points\n"
                    "in %d strokes; %d timed runs after a warm-up, medians, all legs in one job on one box; a HIP-event window holds %d calls\n"
                    "and is divided by that number.\n\n" % (out["device"], out["cpus"], N, P, T, args.repeats, args.group))
            f.write("data on the device                                                        median ms   every run\n")
            f.write("  device-to-device copy of %4d MiB: %7.1f GB/s read + written             %9.4f   %s\n"
                    % (args.copy_mib, out["copy"]["gb_per_s"], out["copy"]["ms"], out["copy"]["ms_all"]))
            f.write("  skf_stroke_table: count launch + offsets scan + write launch            %9.4f   %s\n" % (out["table"]["ms"], out["table"]["ms_all"]))
            f.write("  ops.stroke_table (allocations and the 8-byte read-back included)        %9.4f   %s\n"
                    % (out["table_end_to_end"]["ms"], out["table_end_to_end"]["ms_all"]))
            f.write("  for scale: ops.stroke3_simplify at epsilon 2 (the same walk + RDP)      %9.4f   %s\n"
                    % (out["simplify_for_scale"]["ms"], out["simplify_for_scale"]["ms_all"]))
            for name, title in (("permute", "one random permutation of every sketch"), ("leave_one_out", "leave-one-stroke-out of every sketch")):
                leg = out[name]
                f.write("%s: %d output sketches, %d entries, %d rows (%.2f x the points)\n" % (title, leg["outputs"], leg["entries"], leg["rows"], leg["rows"] / P))
                f.write("  count phase: count launch + offsets scan                                %9.4f   %s\n" % (leg["count_phase"]["ms"], leg["count_phase"]["ms_all"]))
                f.write("  emit launch alone                                                       %9.4f   %s\n" % (leg["emit"]["ms"], leg["emit"]["ms_all"]))
                f.write("    = %.1f MB (12 B a row read, 12 B written, 16 B an entry) at %.1f GB/s: %.1f %% of the copy rate above\n"
                        % (leg["emit"]["bytes"] / 1e6, leg["emit"]["gb_per_s"], 100.0 * leg["emit"]["gb_per_s"] / out["copy"]["gb_per_s"]))
                f.write("  ops.stroke_edit, table given (allocations, the read-back of P')         %9.4f   %s\n" % (leg["end_to_end"]["ms"], leg["end_to_end"]["ms_all"]))
            h = out["host"]
            f.write("\nhost restatement (numpy), both edits of the first %d drawings = %d rows: %.4f s\n" % (h["sketches"], h["rows"], h["s"]))
            f.write("  rows per second, count phases + emit launches over the host: %.1f x; bit-equal to it on those drawings: %s\n"
                    % (out["launches_over_host"], out["bit_equal_on_host_subset"]))
            f.write("Not measured: the packing of a list of drawings into one array and the copies between host and device.\n\n")
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
