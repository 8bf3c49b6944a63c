#!/usr/bin/env python
"""Times teacher-forced scoring (ops.sequence_score over skf_score.hip: the length scan, the row kernel and the sequence sum, three
launches) against the torch composition it replaces on the same tensors - log_softmax + gather + masked sum for the
log-likelihood, (z > z_y).sum for the rank - at the sizes a user runs: cfg-2 (128 x 199 x 1004) and grid tokens
(128 x 199 x 10004), each with QuickDraw-like lengths (synthetic.token_batch) and with every sequence full-length.

Device times are HIP events around groups of --group calls after a warm-up, the median over --repeats, divided by the group
size.  Bytes = the logits of the scored rows (n_b rows of V elements per sample), which the kernel reads once; their rate is set
against the achievable HBM rate of the MI355X (6.3 TB/s).  The composition reads all B * T rows, several times.  The timed
inputs are checked against the float64 restatement of tests/score_reference.py first (a few sequences).  No pass mark: the baseline
is the composition measured in the same run.  Out goes ONE JSON line; with --record also a text record (profiles/score_bench.txt).

    python tools/score_bench.py --record profiles/score_bench.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12      # bytes / s


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


def composition(logits, target, seq_len):
    """what a caller would write without the kernel: every row of the logits, three passes"""
    import torch
    B, T, V = logits.shape
    y = target.clamp(0, V - 1)
    mask = torch.arange(T, device=logits.device)[None, :] < seq_len[:, None]
    lsm = torch.log_softmax(logits.float(), dim=-1)
    tok_logp = lsm.gather(2, y[..., None])[..., 0] * mask
    seq_logp = tok_logp.sum(1)
    zy = logits.gather(2, y[..., None])
    rank = (logits > zy).sum(-1)
    return tok_logp, rank, seq_logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq-len", type=int, default=200)
    ap.add_argument("--vocabs", default="1004,10004")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--group", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import score_reference as ref
    from sketchformer_amd import ops, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs the GPU: nothing here is measured on the host alone")
    B, L = args.batch, args.seq_len
    T = L - 1
    out = {"batch": B, "positions": T, "device": torch.cuda.get_device_name(0), "hbm_achievable_TBps": HBM_ACHIEVABLE / 1e12, "cases": []}
    for V in (int(v) for v in args.vocabs.split(",")):
        for dtype in args.dtypes.split(","):
            esz = 2 if dtype == "bf16" else 4
            ld = (V + 7) // 8 * 8 if dtype == "bf16" else V           # the pitch of the model's own buffer
            gen = torch.Generator(device="cuda").manual_seed(V)
            buf = torch.empty(B * T, ld, dtype=torch.float32, device="cuda").normal_(0.0, 3.0, generator=gen)
            buf = buf.to(torch.bfloat16) if dtype == "bf16" else buf
            logits = buf[:, :V]
            eos = V - 1
            for lengths in ("quickdraw", "full"):
                x, _ = synthetic.token_batch(B, L, V, 345, seed=0, full=lengths == "full")
                if lengths == "full":
                    x[:, -1] = eos                                       # (truncated rows lose their EOS: every position is scored either way)
                target = torch.from_numpy(x).cuda()
                fn = lambda: ops.sequence_score(logits, target, eos, tgt_off=1, T=T)      # noqa: E731
                tok_logp, tok_rank, seq_logp, seq_len = fn()
                n = seq_len.cpu().numpy()
                for b in (0, B // 2, B - 1):                             # the timed inputs give the restatement's results
                    z = logits.view(B, T, V)[b].float().cpu().numpy()
                    wlp, wrk, ws, wn = ref.sequence_score(z[None], x[b:b + 1, 1:], eos)
                    assert wn[0] == n[b] and np.array_equal(wrk[0], tok_rank[b].cpu().numpy())
                    assert np.abs(tok_logp[b].cpu().numpy() - wlp[0]).max() <= ref.logp_bound(z, V)
                view3 = logits.unflatten(0, (B, T))
                comp = lambda: composition(view3, target[:, 1:], seq_len)     # noqa: E731
                c_lp, c_rank, _ = comp()
                assert (c_lp - tok_logp).abs().max().item() <= 1e-3
                us, all_us = timed(fn, args.group, args.repeats, args.warmup)
                cus, call_us = timed(comp, max(args.group // 5, 1), args.repeats, args.warmup)
                scored_bytes = int(n.sum()) * V * esz
                out["cases"].append({
                    "V": V, "dtype": dtype, "lengths": lengths, "scored_rows": int(n.sum()), "rows": B * T, "scored_bytes": scored_bytes,
                    "kernel_us": us, "kernel_repeats_us": all_us, "composition_us": cus, "composition_repeats_us": call_us,
                    "speedup": round(cus / us, 2), "scored_TBps": round(scored_bytes / (us * 1e-6) / 1e12, 3),
                    "hbm_share": round(scored_bytes / (us * 1e-6) / HBM_ACHIEVABLE, 3)})
            del buf, logits
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.record:
        with open(args.record, "w") as f:
            f.write("tools/score_bench.py on %s: HIP events, median of %d repeats (groups of %d calls, %d warm-up calls)\n"
                    % (out["device"], args.repeats, args.group, args.warmup))
            f.write("B = %d sequences of T = %d scored positions; kernel = ops.sequence_score (three launches: length scan, rows, sequence sum);\n"
                    "composition = torch log_softmax + gather + masked sum, and (z > z_y).sum for the rank, on the same tensors\n"
                    "bytes = the logits of the scored rows, read once; share = their rate over the achievable HBM rate of %.1f TB/s\n"
                    "(a tensor of up to 256 MiB can be served by the Infinity Cache between calls: a share above 1 says so)\n\n"
                    % (B, T, HBM_ACHIEVABLE / 1e12))
            f.write("%6s %5s %10s %12s %12s %12s %14s %9s %8s %7s\n" % ("V", "dtype", "lengths", "scored rows", "scored MB", "kernel (us)",
                                                                      "composition(us)", "speed-up", "TB/s", "share"))
            for c in out["cases"]:
                f.write("%6d %5s %10s %12d %12.1f %12.2f %14.2f %9.2f %8.3f %7.3f\n" % (
                    c["V"], c["dtype"], c["lengths"], c["scored_rows"], c["scored_bytes"] / 1e6, c["kernel_us"], c["composition_us"],
                    c["speedup"], c["scored_TBps"], c["hbm_share"]))
            f.write("\nrepeats (us), kernel / composition:\n")
            for c in out["cases"]:
                f.write("  V %d %s %s: %s / %s\n" % (c["V"], c["dtype"], c["lengths"], c["kernel_repeats_us"], c["composition_repeats_us"]))
            slower = [c for c in out["cases"] if c["V"] == 1004 and c["speedup"] < 1.0]
            if slower:
                f.write("\nNOT faster than the composition at V = 1004 in: %s\n" % ", ".join("%s %s" % (c["dtype"], c["lengths"]) for c in slower))
            build = os.path.join(ROOT, "profiles", "score_build.txt")
            if os.path.exists(build):                              # registers and LDS of the kernels as compiled
                with open(build) as b:
                    f.write("\n" + b.read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
