"""Prefix-forced greedy decoding as include/skf.h states it (skf_model_prefix_decode), in float64 numpy over a logits callback: forced
positions emit their prefix token and ask for no logits, free positions take the first arg-max, a token outside [0, vocab) counts
as PAD, EOS flags are sticky and a forced EOS counts, and the decode ends after the first position behind which every one of the
n_valid rows has an EOS.  The device tests are held to this file; it knows nothing of the device."""
import numpy as np

PAD = 0


def forced_token(prefix, prefix_len, b, s, vocab):
    """the token position s of row b is forced to, or None where the position is free"""
    if s >= int(prefix_len[b]):
        return None
    t = int(prefix[b][s])
    return PAD if t < 0 or t >= vocab else t


def forced_greedy(logits_fn, prefix, prefix_len, sos, eos, max_steps, vocab, n_valid=None, on_free=None):
    """logits_fn(tokens (n, s + 1) int64) -> (n, V) logits of position s for every row (rows whose position is forced are ignored).
    on_free(b, s, logits row, token): called for every free position, in decoding order.
    Returns (tokens (n, columns) int64 incl. the start symbol, forced (n, columns) bool: column s + 1 was forced)."""
    prefix_len = np.asarray(prefix_len).reshape(-1)
    n = len(prefix_len)
    n_valid = n if n_valid is None else n_valid
    out = np.full((n, 1), sos, dtype=np.int64)
    forced = np.zeros((n, 1), dtype=bool)
    seen = np.zeros(n, dtype=bool)
    for s in range(max_steps):
        want = [forced_token(prefix, prefix_len, b, s, vocab) for b in range(n)]
        logits = None
        if any(w is None for w in want):
            logits = np.asarray(logits_fn(out), dtype=np.float64)
        col = np.zeros(n, dtype=np.int64)
        for b in range(n):
            if want[b] is None:
                col[b] = int(np.argmax(logits[b]))              # the first index on ties
                if on_free is not None:
                    on_free(b, s, logits[b], int(col[b]))
            else:
                col[b] = want[b]
        out = np.concatenate([out, col[:, None]], axis=1)
        forced = np.concatenate([forced, np.array([w is not None for w in want])[:, None]], axis=1)
        seen |= col == eos
        if seen[:n_valid].all():
            break
    return out, forced
