"""Float64 restatement of the teacher-forced scoring rule (include/skf.h: skf_sequence_score), numpy only.

    scored_length(y, eos)            n_b: (first position with y == eos) + 1, else the first position with y == 0, else T
    token_score(z, y)                (log p, rank) of one row: log p = z_y - m - log sum exp(z - m); rank = #{z_j > z_y} + #{j < y: z_j == z_y};
                                     a target outside [0, V) scores (-inf, V); a -inf target under a finite maximum scores -inf
    sequence_score(logits, target, eos)
                                     tok_logp (B, T) float64 (0.0 behind n_b), tok_rank (B, T) int (-1 behind n_b), seq_logp (B) float64
                                     = the sum of the scored tok_logp in ascending t, seq_len (B) int.  Rows at t >= n_b are not
                                     touched: they may hold NaN.
    sequential_sum_f32(tok_logp, n)  the float32 sum the device stores in seq_logp: one rounding per added position, from 0.0f
    logp_bound(z, V)                 the float32 error bound of one tok_logp (derived in tests/test_gpu_score.py)
"""
import numpy as np


def scored_length(y, eos):
    y = np.asarray(y)
    hit = np.nonzero(y == eos)[0]
    if len(hit):
        return int(hit[0]) + 1
    pad = np.nonzero(y == 0)[0]
    return int(pad[0]) if len(pad) else len(y)


def token_score(z, y):
    z = np.asarray(z, dtype=np.float64)
    V = len(z)
    y = int(y)
    if y < 0 or y >= V:
        return -np.inf, V
    zy = z[y]
    rank = int(np.sum(z > zy)) + int(np.sum(z[:y] == zy))
    m = z.max()
    if zy == -np.inf:                                     # (finite m: the contract) never -inf - -inf
        return -np.inf, rank
    return float((zy - m) - np.log(np.sum(np.exp(z - m)))), rank


def sequence_score(logits, target, eos):
    """logits (B, T, V) any float dtype (used as float64), target (B, T) integers."""
    logits, target = np.asarray(logits), np.asarray(target)
    B, T = target.shape
    tok_logp = np.zeros((B, T), np.float64)
    tok_rank = np.full((B, T), -1, np.int64)
    seq_logp = np.zeros(B, np.float64)
    seq_len = np.zeros(B, np.int64)
    for b in range(B):
        n = scored_length(target[b], eos)
        seq_len[b] = n
        for t in range(n):
            tok_logp[b, t], tok_rank[b, t] = token_score(logits[b, t], target[b, t])
            seq_logp[b] += tok_logp[b, t]
    return tok_logp, tok_rank, seq_logp, seq_len


def sequential_sum_f32(tok_logp, n):
    s = np.float32(0.0)
    with np.errstate(invalid="ignore"):
        for t in range(int(n)):
            s = np.float32(s + np.float32(tok_logp[t]))
    return s


def logp_bound(z, V):
    """16 * 2^-23 * max(1, max|z| over the row's finite entries + ln V)"""
    z = np.asarray(z, dtype=np.float64)
    fin = z[np.isfinite(z)]
    big = float(np.abs(fin).max()) if len(fin) else 0.0
    return 16.0 * 2.0 ** -23 * max(1.0, big + np.log(V))
