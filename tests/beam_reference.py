"""Beam search as include/skf.h states it (skf_beam_advance, skf_model_beam_decode), in float64 numpy: the row's log-softmax and
its W best candidates, the merge of a sketch's offers with its tie order, finished beams, the final order, and the margin of a
step (how far the decision was from going the other way).  The device tests are held to this file; it knows nothing of the device."""
import numpy as np

PAD = 0


def log_softmax(row):
    """log p of one row of logits; NaN counts as -inf, and a row without a finite maximum has no distribution (all -inf)"""
    z = np.asarray(row, dtype=np.float64).copy()
    z[np.isnan(z)] = -np.inf
    m = z.max()
    if not np.isfinite(m):
        return np.full(z.shape, -np.inf)
    return z - (m + np.log(np.exp(z - m).sum()))


def top_w(logp, W):
    """the W best entries of a row: (log p (W,), token (W,)), log p descending, then token ascending"""
    logp = np.asarray(logp, dtype=np.float64)
    order = np.lexsort((np.arange(len(logp)), -logp))[:W]
    return logp[order], order.astype(np.int64)


def offers(scores, finished, cand_lp, cand_tok):
    """Every offer of one sketch, in offer order (parent-major): arrays score, parent, token of W * W entries.  A live beam offers
    score + log p for each of its W candidates; a finished beam offers itself once (its score, PAD) and -inf otherwise."""
    W = len(scores)
    sc = np.full(W * W, -np.inf)
    tok = np.zeros(W * W, dtype=np.int64)
    par = np.repeat(np.arange(W), W)
    for r in range(W):
        for k in range(W):
            if finished[r]:
                if k == 0:
                    sc[r * W] = scores[r]
            else:
                sc[r * W + k] = np.float64(scores[r]) + np.float64(cand_lp[r][k])
                tok[r * W + k] = cand_tok[r][k]
    sc[np.isnan(sc)] = -np.inf
    return sc, par, tok


def merge(scores, finished, lengths, cand_lp, cand_tok, step, eos):
    """One step of one sketch.  Returns (survivors, ranked): survivors = dict of (W,) arrays parent, token, score, finished, length,
    best first; ranked = every offer's score in rank order (score descending, parent ascending, token ascending, offer index)."""
    W = len(scores)
    sc, par, tok = offers(scores, finished, cand_lp, cand_tok)
    order = np.lexsort((np.arange(W * W), tok, par, -sc))
    keep = order[:W]
    pfin = np.asarray(finished, dtype=bool)[par[keep]]
    out = dict(parent=par[keep], token=tok[keep], score=sc[keep],
               finished=(pfin | (tok[keep] == eos)).astype(np.int32),
               length=np.where(pfin, np.asarray(lengths)[par[keep]], step + 1).astype(np.int32))
    return out, sc[order]


def margin(ranked, W):
    """Smallest gap between adjacent ranks 1 .. W + 1 of a step's ranked offers: below it a perturbation of the scores can change
    who survives or in which order.  A gap to -inf (or past the last offer) is infinite."""
    s = np.asarray(ranked, dtype=np.float64)
    gaps = []
    for i in range(min(W, len(s) - 1)):
        gaps.append(np.inf if not np.isfinite(s[i + 1]) or not np.isfinite(s[i]) else s[i] - s[i + 1])
    return min(gaps) if gaps else np.inf


def next_ancestry(anc, parent, step, base=0):
    """rows of the next table of one sketch: the parent's row up to `step`, then the row's own slot (base + r')"""
    anc = np.asarray(anc)
    out = np.zeros_like(anc)
    for r, p in enumerate(parent):
        out[r, :step + 1] = anc[p, :step + 1]
        out[r, step + 1] = base + r
    return out


def final_order(scores, lengths, alpha):
    """beam indices by score / ((5 + len) / 6)^alpha descending, then beam index ascending"""
    s = np.asarray(scores, dtype=np.float64)
    ns = s if alpha == 0 else s / ((5.0 + np.asarray(lengths, dtype=np.float64)) / 6.0) ** alpha
    ns = np.where(np.isnan(ns), -np.inf, ns)
    return np.lexsort((np.arange(len(s)), -ns))


def beam_search(logits_fn, W, sos, eos, max_steps, alpha=0.0):
    """The whole search of ONE sketch.  logits_fn(prefixes (W, t + 1) int64) -> (W, V) logits of position t for every beam.
    Returns dict(tokens (W, T) in final order, scores, lengths, finished, min_margin, steps) with T = steps + 1; the search ends
    after max_steps positions or once every beam is finished."""
    hyp = np.full((W, 1), sos, dtype=np.int64)
    scores = np.full(W, -np.inf)
    scores[0] = 0.0
    finished = np.zeros(W, dtype=np.int32)
    lengths = np.zeros(W, dtype=np.int32)
    worst = np.inf
    steps = 0
    for step in range(max_steps):
        if finished.all():
            break
        logits = np.asarray(logits_fn(hyp), dtype=np.float64)
        cl, ct = zip(*(top_w(log_softmax(logits[r]), W) for r in range(W)))
        s, ranked = merge(scores, finished, lengths, cl, ct, step, eos)
        worst = min(worst, margin(ranked, W))
        hyp = np.concatenate([hyp[s["parent"]], s["token"][:, None]], axis=1)
        scores, finished, lengths = s["score"], s["finished"], s["length"]
        steps = step + 1
    order = final_order(scores, lengths, alpha)
    return dict(tokens=hyp[order], scores=scores[order], lengths=lengths[order], finished=finished[order], min_margin=worst, steps=steps)
