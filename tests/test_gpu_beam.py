"""Beam-search reconstruction on the device (include/skf.h: the selection rule; skf_beam.hip, decode_position_kernel<.., BEAM>).

The merge kernel is held to tests/beam_reference.py (float64) on hand-made offers; the model-level search is held to the oracle:
every returned hypothesis carries the oracle's teacher-forced log-likelihood, and the restatement's own float64 search on oracle
logits returns the same hypotheses wherever the oracle's margins decide it.  The embeddings of the oracle test are random vectors
made here from `ORACLE_SEEDS`."""
import numpy as np
import pytest
import torch

import oracle
from oracle import sketchformer_oracle
import beam_reference as ref
from test_gpu_decode_attention import CFG2, SMALL, SMALL16, _build, _inputs, _params

pytestmark = pytest.mark.gpu

MAX_STEPS = 12                       # of the oracle test: tau = 4e-4 * MAX_STEPS
PAD_NUDGE, EOS_NUDGE = 3.0, 2.0      # output-bias nudges, as in the sampling test
# (blind, B, W) -> seed of the embeddings.  With these, in every case at least 3 in 4 sketches are decidable and at least one
# decidable sketch has a best hypothesis that is not the greedy row
ORACLE_SEEDS = {(True, 8, 2): 5, (True, 8, 4): 112, (True, 6, 2): 5, (True, 6, 4): 7,
                (False, 8, 2): 18, (False, 8, 4): 26, (False, 6, 2): 5, (False, 6, 4): 7}


def _sos_eos(ocfg):
    return ocfg.vocab_size - 2, ocfg.vocab_size - 1


def _first_eos(row, eos):
    hit = np.nonzero(np.asarray(row)[1:] == eos)[0]
    return int(hit[0]) + 1 if len(hit) else len(row)


# ---------------------------------------------------------------- 1. the merge kernel against the restatement
def _anc(rng, n, W, step, ld):
    a = np.zeros((n * W, ld), dtype=np.int32)
    for g in range(n):
        a[g * W:(g + 1) * W, :step] = g * W + rng.randint(0, W, size=(W, step))
    a[:, step] = np.arange(n * W)
    return a


def merge_case(W, V, n, step, kind, seed):
    """Offers of n sketches: dict of float32 / int32 arrays (what the device gets) - built on the host alone.
    kind: plain | all_finished | finished_leads | neg_inf | ties"""
    rng = np.random.RandomState(seed)
    R = n * W
    lp = np.zeros((R, W), np.float32)
    tk = np.zeros((R, W), np.int32)
    for r in range(R):
        a, b = ref.top_w(ref.log_softmax(rng.randn(V) * 3.0), W)
        lp[r], tk[r] = a, b
    scores = (-rng.uniform(2.0, 18.0, size=R)).astype(np.float32)
    fin = np.zeros(R, np.int32)
    ln = np.zeros(R, np.int32)
    if step == 0:
        scores[:] = -np.inf
        scores[::W] = 0.0
    elif kind == "all_finished":
        fin[:] = 1
    elif kind == "finished_leads" and W > 1:
        fin[::W] = 1
        scores[::W] = -0.5                                            # above every live offer
    if kind == "neg_inf":
        lp[:, W // 2 + 1:] = -np.inf                                  # the tail of every beam's candidates
        if step and W > 2:
            scores[1::W] = -np.inf                                    # and a dead beam
    if kind == "ties" and step and W > 1:
        for g in range(n):                                            # beams 0 and 1 of a sketch: the same row, the same score
            lp[g * W + 1], tk[g * W + 1], scores[g * W + 1] = lp[g * W], tk[g * W], scores[g * W]
            if W > 2 and V > W:                                       # and two tokens of beam 2 with the same log p
                lp[g * W + 2, 1] = lp[g * W + 2, 0]
                tk[g * W + 2, :2] = np.sort(tk[g * W + 2, :2])
    ln[fin > 0] = rng.randint(1, step + 1, size=int(fin.sum())) if step else 0
    return dict(lp=lp, tk=tk, scores=scores, fin=fin, ln=ln, anc=_anc(rng, n, W, step, step + 3))


def merge_cases(W, V, n):
    """[(name, step, case)]; the non-tie cases are regenerated until the restatement's smallest gap is >= 1e-3"""
    out = []
    for step, kind in ((0, "plain"), (0, "neg_inf"), (3, "plain"), (7, "all_finished"), (5, "finished_leads"), (4, "neg_inf"),
                       (6, "ties")):
        seed = 1000 * W + V + 17 * n + step
        while True:
            c = merge_case(W, V, n, step, kind, seed)
            if kind == "ties" or _case_margin(c, W, n, step) >= 1e-3:
                break
            seed += 7919
        out.append(("%s_step%d" % (kind, step), step, c))
    return out


def _expect(c, W, n, step, eos):
    res, ranked = [], []
    for g in range(n):
        sl = slice(g * W, (g + 1) * W)
        s, rk = ref.merge(c["scores"][sl], c["fin"][sl], c["ln"][sl], c["lp"][sl], c["tk"][sl], step, eos)
        s["anc"] = ref.next_ancestry(c["anc"][sl], s["parent"], step, base=g * W)
        res.append(s)
        ranked.append(rk)
    return res, ranked


def _case_margin(c, W, n, step):
    return min(ref.margin(rk, W) for rk in _expect(c, W, n, step, eos=-1)[1])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("V", [8, 52, 1004])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_beam_step_follows_the_rule(W, V, n):
    from sketchformer_amd import ops
    worst = 0.0
    for name, step, c in merge_cases(W, V, n):
        eos = int(c["tk"][0, 0])                                     # a token that does occur among the offers
        want, ranked = _expect(c, W, n, step, eos)
        if not name.startswith("ties"):
            assert min(ref.margin(rk, W) for rk in ranked) >= 1e-3, name       # on the CPU values
        dev = lambda a: torch.from_numpy(a).cuda()                   # noqa: E731
        got = ops.beam_step(dev(c["lp"]), dev(c["tk"]), dev(c["scores"]), dev(c["fin"]), dev(c["anc"]), step, eos, lengths=dev(c["ln"]))
        got = {k: v.cpu().numpy() for k, v in got.items()}
        for g in range(n):
            sl = slice(g * W, (g + 1) * W)
            w = want[g]
            assert np.array_equal(got["parent"][sl], w["parent"]), (name, g, got["parent"][sl], w["parent"])
            assert np.array_equal(got["token"][sl], w["token"]), (name, g)
            assert np.array_equal(got["pad"][sl], (w["token"] == 0).astype(np.uint8)), (name, g)
            assert np.array_equal(got["finished"][sl], w["finished"]), (name, g)
            assert np.array_equal(got["length"][sl], w["length"]), (name, g)
            assert np.array_equal(got["anc"][sl, :step + 2], w["anc"][:, :step + 2]), (name, g)
            fin = np.isfinite(w["score"])
            assert np.array_equal(np.isfinite(got["score"][sl]), fin) and (got["score"][sl][~fin] == -np.inf).all(), (name, g)
            if fin.any():
                rel = np.abs(got["score"][sl][fin] - w["score"][fin]) / np.maximum(np.abs(w["score"][fin]), 1.0)
                worst = max(worst, float(rel.max()))
                assert rel.max() <= 1e-5, (name, g, rel.max())
    print("W=%d V=%d n=%d: worst relative score error %.3g" % (W, V, n, worst))


# ---------------------------------------------------------------- 2. beam_width = 1 is greedy
def _assert_width_one_is_greedy(eng, emb, el, sos, eos):
    want = eng.greedy_decode(emb, expected_len=el, sos=sos, eos=eos)
    tok, score, length = eng.beam_decode(emb, expected_len=el, sos=sos, eos=eos, beam_width=1)
    assert tok.shape[:2] == (want.shape[0], 1) and tok.dtype == np.int32 and score.dtype == np.float32 and length.dtype == np.int32
    for r in range(want.shape[0]):
        k = min(_first_eos(want[r], eos) + 1, want.shape[1], tok.shape[2])
        assert _first_eos(tok[r, 0], eos) == _first_eos(want[r], eos) or tok.shape[2] < want.shape[1]
        assert np.array_equal(tok[r, 0, :k], want[r, :k]), (r, tok[r, 0, :k], want[r, :k])
        assert length[r, 0] == min(_first_eos(tok[r, 0], eos), tok.shape[2] - 1)
        assert np.isfinite(score[r, 0]) and score[r, 0] <= 0


@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_width_one_is_greedy_small(blind):
    eng, ocfg = _build(4, blind=blind)
    emb, tlen = _inputs(eng, ocfg, 4, seed=8)
    b = eng.get("output/bias").copy()
    b[ocfg.vocab_size - 1] += 1.0                 # rows end at different positions
    eng.set("output/bias", b)
    el = tlen if not blind else None
    if not blind:
        el = np.maximum(tlen, 1)
    _assert_width_one_is_greedy(eng, emb, el, *_sos_eos(ocfg))


def test_width_one_is_greedy_head_size_64():
    eng, ocfg = _build(4, blind=True, **SMALL16)
    emb, _ = _inputs(eng, ocfg, 4, seed=7)
    _assert_width_one_is_greedy(eng, emb, None, *_sos_eos(ocfg))


def test_width_one_is_greedy_cfg2_dimensions():
    from sketchformer_amd import engine, synthetic
    B = 8
    eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.0, use_graph=False, seed=1, **CFG2), init_seed=2)
    x, _ = synthetic.token_batch(B, CFG2["seq_len"], CFG2["vocab_size"], CFG2["n_classes"], seed=0)
    eng.encode(x)
    emb = eng.buffer("embedding").float().clone()
    V = CFG2["vocab_size"]
    _assert_width_one_is_greedy(eng, emb, None, V - 2, V - 1)


def test_width_one_is_greedy_bf16_model():
    eng, ocfg = _build(4, blind=True, act_dtype="bf16", **SMALL16)
    emb, _ = _inputs(eng, ocfg, 4, seed=7)
    _assert_width_one_is_greedy(eng, emb, None, *_sos_eos(ocfg))


# ---------------------------------------------------------------- 3. model beam search against the oracle
def _teacher_forced_logits(P, ocfg, emb, recon, expected_len):
    """the oracle's logits of every position on the given prefix: (n, T, V), T = recon length - 1"""
    T = recon.shape[1] - 1
    tar = recon[:, :T]
    nattn = expected_len if expected_len is not None else T
    dummy = sketchformer_oracle.make_dummy_input(ocfg, expected_len, nattn, emb.shape[0])
    _, combined, dec_pad = sketchformer_oracle.create_masks(dummy, tar)
    return sketchformer_oracle.decode(P, ocfg, np.asarray(emb, np.float64), tar, dec_pad, combined)


def oracle_inputs(blind, B, W):
    """the embeddings (and lengths) of one oracle case: random vectors, made on the host"""
    rng = np.random.RandomState(100 + ORACLE_SEEDS[(blind, B, W)])
    n = B // W
    emb = (rng.randn(n, SMALL["d_model"]) * 0.5).astype(np.float32)      # attn_version 1: the embedding has d_model columns
    el = None if blind else rng.randint(3, SMALL["seq_len"], size=n).astype(np.int32)
    return emb, el


def nudge(bias, eos):
    b = np.array(bias, copy=True)
    b[0] += PAD_NUDGE
    b[eos] += EOS_NUDGE
    return b


def oracle_search(P, ocfg, emb_g, el_g, W, sos, eos, alpha=0.0):
    """the restatement's float64 beam search of one sketch on oracle logits"""
    e = np.repeat(np.asarray(emb_g, np.float64)[None], W, axis=0)
    el = None if el_g is None else np.repeat(el_g, W)

    def fn(prefixes):
        recon = np.concatenate([prefixes, np.zeros((W, 1), np.int64)], axis=1)
        return _teacher_forced_logits(P, ocfg, e, recon, el)[:, -1]
    return ref.beam_search(fn, W, sos, eos, MAX_STEPS, alpha)


@pytest.mark.parametrize("B", [8, 6])
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_beam_search_against_the_oracle(blind, W, B):
    eng, ocfg = _build(B, blind=blind)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    P = _params(eng)
    emb, el = oracle_inputs(blind, B, W)
    n = B // W
    tok, score, length = eng.beam_decode(emb, expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS, beam_width=W)
    T = tok.shape[2]
    assert tok.shape == (n, W, T) and score.shape == (n, W) and length.shape == (n, W) and (tok[:, :, 0] == sos).all()
    img = eng.buffer("decode/tokens").contiguous().view(torch.int64).cpu().numpy()          # (B, L + 1)
    anc = eng.buffer("decode/ancestry").contiguous().view(torch.int32).cpu().numpy()          # (B, L + 1): the table the gather read
    pads = early = 0
    worst = 0.0
    for g in range(n):
        # (a) every hypothesis: score, length, EOS position, and the gather through the ancestry
        e = np.repeat(emb[g:g + 1], W, axis=0)
        lg = _teacher_forced_logits(P, ocfg, e, np.concatenate([tok[g], np.zeros((W, 1), tok.dtype)], axis=1).astype(np.int64),
                                    None if el is None else np.repeat(el[g], W))
        reread = set()
        for k in range(W):
            row = tok[g, k]
            fe = _first_eos(row, eos)
            assert length[g, k] == min(fe, T - 1), (g, k, row, length[g, k])
            assert (row[fe + 1:] == 0).all()                          # PADs behind the EOS
            want = sum(ref.log_softmax(lg[k, i])[row[i + 1]] for i in range(length[g, k]))
            err = abs(want - float(score[g, k]))
            worst = max(worst, err / max(int(length[g, k]), 1))
            assert err <= 2e-4 * length[g, k], (g, k, want, score[g, k], length[g, k])
            pads += int((row[1:length[g, k]] == 0).sum())
            early += int(fe < T - 1)
            r = g * W + k
            reread.add(tuple(int(img[anc[r, j], j]) for j in range(T)))
        assert reread == set(tuple(int(v) for v in tok[g, k]) for k in range(W)), g
        assert (np.diff(score[g]) <= 0).all()                         # alpha = 0: ranked by the raw sum
    # (b) the restatement's own search on oracle logits, wherever its margins decide
    tau = 4e-4 * MAX_STEPS
    decidable = differs = 0
    pad_e = np.zeros((B,) + emb.shape[1:], np.float32)
    pad_e[:n] = emb
    greedy = eng.greedy_decode(pad_e, expected_len=None if el is None else np.concatenate([el, np.ones(B - n, el.dtype)]), n_valid=n,
                               sos=sos, eos=eos, max_steps=MAX_STEPS)
    for g in range(n):
        s = oracle_search(P, ocfg, emb[g], None if el is None else el[g], W, sos, eos)
        if s["min_margin"] < tau:
            continue
        decidable += 1
        kg = min(_first_eos(greedy[g], eos) + 1, greedy.shape[1])      # the device's best row against the device's greedy row
        best = tok[g, 0, :min(_first_eos(tok[g, 0], eos) + 1, T)]
        differs += int(len(best) != kg or not np.array_equal(best, greedy[g, :kg]))
        k = min(T, s["tokens"].shape[1])
        assert np.array_equal(tok[g][:, :k], s["tokens"][:, :k]), (g, tok[g], s["tokens"])
        assert (tok[g][:, k:] == 0).all() and (s["tokens"][:, k:] == 0).all()
        assert np.array_equal(length[g], s["lengths"]), g
    print("blind=%s B=%d W=%d: %d of %d sketches decidable, %d of them where the device's best beam != its greedy row, %d PADs inside hypotheses, %d early ends, "
          "worst score error per position %.3g" % (blind, B, W, decidable, n, differs, pads, early, worst))
    assert 4 * decidable >= 3 * n, (decidable, n)
    assert differs >= 1


def test_oracle_cases_read_the_mask_through_the_ancestry():
    """over the oracle cases some hypothesis holds a PAD inside (so a masked key is read through another slot) and some end early;
    counted on the device's own output of one case"""
    eng, ocfg = _build(8, blind=True)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    emb, _ = oracle_inputs(True, 8, 4)
    tok, _, length = eng.beam_decode(emb, sos=sos, eos=eos, max_steps=MAX_STEPS, beam_width=4)
    pads = sum(int((tok[g, k, 1:length[g, k]] == 0).sum()) for g in range(2) for k in range(4))
    ends = int((length < tok.shape[2] - 1).sum())
    assert pads >= 1 and ends >= 1, (pads, ends)


# ---------------------------------------------------------------- 4. determinism and isolation
def test_determinism_and_isolation():
    B, W = 8, 4
    eng, ocfg = _build(B, blind=True)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    full, _ = _inputs(eng, ocfg, B, seed=8)
    kw = dict(sos=sos, eos=eos, beam_width=W)
    g_before = eng.greedy_decode(full, sos=sos, eos=eos)
    s_before = eng.sample_decode(full, sos=sos, eos=eos, top_k=1, seed=3)
    emb = full[:2]
    a = eng.beam_decode(emb, **kw)
    b = eng.beam_decode(emb, **kw)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)              # bit-equal: tokens, scores, lengths
    # the same sketch in the other group slot, next to another neighbour
    c = eng.beam_decode(np.stack([full[5], emb[0]]), **kw)
    for x, y in zip(a, c):
        k = min(x.shape[-1], y.shape[-1]) if x.ndim == 3 else None
        if x.ndim == 3:
            n_ = [min(_first_eos(x[0, h], eos) + 1, k) for h in range(W)]
            assert all(np.array_equal(x[0, h, :n_[h]], y[1, h, :n_[h]]) for h in range(W))
        else:
            assert np.array_equal(x[0], y[1])
    assert np.array_equal(eng.greedy_decode(full, sos=sos, eos=eos), g_before)
    assert np.array_equal(eng.sample_decode(full, sos=sos, eos=eos, top_k=1, seed=3), s_before)


# ---------------------------------------------------------------- 5. stop rule and length_alpha
def test_stop_rule_and_frozen_scores():
    B, W = 8, 2
    eng, ocfg = _build(B, blind=True)
    sos, eos = _sos_eos(ocfg)
    b = eng.get("output/bias").copy()
    b[eos] += 6.0                                  # EOS is the best or second best token of nearly every position
    eng.set("output/bias", b)
    full, _ = _inputs(eng, ocfg, B, seed=8)
    emb = full[:4]
    tok, score, length = eng.beam_decode(emb, sos=sos, eos=eos, beam_width=W, n_valid=3)
    T = tok.shape[2]
    fe = np.array([[_first_eos(tok[g, k], eos) for k in range(W)] for g in range(3)])
    assert (fe < T).all() and fe.max() == T - 1, (fe, T)              # out_len: the first position after which all have ended
    assert T - 1 < ocfg.seq_len
    for g in range(3):
        for k in range(W):
            assert length[g, k] == fe[g, k] and (tok[g, k, fe[g, k] + 1:] == 0).all()


def test_finished_hypotheses_keep_their_scores_while_others_go_on():
    """the oracle case (blind, 8, 2): a sketch whose beams have all ended early is decoded first alone in the stop test (n_valid = 1:
    the call ends with it), then with the others (the call goes on): its hypotheses, scores and lengths are the same"""
    B, W = 8, 2
    eng, ocfg = _build(B, blind=True)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    emb, _ = oracle_inputs(True, B, W)
    kw = dict(sos=sos, eos=eos, max_steps=MAX_STEPS, beam_width=W)
    tok, score, length = eng.beam_decode(emb, **kw)
    T = tok.shape[2]
    ends = np.array([max(_first_eos(tok[g, k], eos) for k in range(W)) for g in range(B // W)])
    g0 = int(np.argmin(ends))
    assert ends[g0] < T - 1, (ends, T)                                # all its beams end before the call does
    first = np.concatenate([emb[g0:g0 + 1], np.delete(emb, g0, axis=0)])
    tok1, score1, length1 = eng.beam_decode(first, n_valid=1, **kw)
    assert tok1.shape[2] == ends[g0] + 1 < T                          # the short call really is shorter
    assert np.array_equal(score1[0], score[g0]) and np.array_equal(length1[0], length[g0])
    assert np.array_equal(tok1[0], tok[g0][:, :tok1.shape[2]]) and (tok[g0][:, tok1.shape[2]:] == 0).all()


def test_length_alpha_reorders_and_keeps_the_scores():
    B, W = 8, 4
    eng, ocfg = _build(B, blind=True)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    full, _ = _inputs(eng, ocfg, B, seed=8)
    emb = full[:2]
    t0, s0, l0 = eng.beam_decode(emb, sos=sos, eos=eos, beam_width=W, length_alpha=0.0)
    compared = 0
    for alpha in (1.0, 3.0, 8.0):
        t1, s1, l1 = eng.beam_decode(emb, sos=sos, eos=eos, beam_width=W, length_alpha=alpha)
        for g in range(2):
            order = ref.final_order(s0[g], l0[g], alpha)              # beam index = the rank at alpha = 0
            ns = s0[g].astype(np.float64) / ((5.0 + l0[g]) / 6.0) ** alpha
            gaps = np.abs(np.diff(np.sort(ns)))
            if gaps.min() < 1e-4 * np.abs(ns).max():                 # too close for fp32 to order like float64
                continue
            assert np.array_equal(s1[g], s0[g][order]) and np.array_equal(l1[g], l0[g][order])      # the raw sums, reordered
            assert np.array_equal(t1[g], t0[g][order])
            compared += 1
    assert compared >= 1


def test_length_alpha_reorders_a_constructed_pair():
    """skf_beam_finish on hand-made beams: a short hypothesis with the higher sum against a long one with a lower sum.
    -2.0 / ((5 + 1) / 6) = -2.0 against -2.4 / ((5 + 9) / 6) = -1.029: alpha = 1 puts the long one first, alpha = 0 the short one;
    the scores handed back are the raw sums either way.  The rows are read through the ancestry (slots crossed on purpose)."""
    from sketchformer_amd import ops
    T = 11
    img = np.zeros((4, T), np.int64)
    img[0] = 100 + np.arange(T)                                       # slot 0 .. 3 of two sketches of two beams
    img[1] = 200 + np.arange(T)
    img[2] = 300 + np.arange(T)
    img[3] = 400 + np.arange(T)
    anc = np.array([[0] * T, [1, 0] + [1] * (T - 2), [3] * 5 + [2] * (T - 5), [3] * T], np.int32)
    rows = np.stack([img[anc[r], np.arange(T)] for r in range(4)])    # what every hypothesis reads
    scores = np.array([-2.0, -2.4, -3.0, -2.9], np.float32)           # sketch 1: no change of order at any alpha here
    lengths = np.array([1, 9, 4, 4], np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()                        # noqa: E731
    for alpha, order0 in ((0.0, [0, 1]), (1.0, [1, 0])):
        assert ref.final_order(scores[:2], lengths[:2], alpha).tolist() == order0
        t, s, ln = (v.cpu().numpy() for v in ops.beam_finish(dev(scores), dev(lengths), dev(anc), dev(img), 2, alpha, ncols=T - 1))
        assert np.array_equal(s[0], scores[:2][order0]) and np.array_equal(ln[0], lengths[:2][order0])      # raw sums, unchanged
        assert np.array_equal(t[0][:, :T - 1], rows[:2][order0][:, :T - 1]) and (t[:, :, T - 1] == 0).all()
        assert np.array_equal(s[1], scores[[3, 2]]) and np.array_equal(ln[1], lengths[[3, 2]])
        assert np.array_equal(t[1][:, :T - 1], rows[[3, 2]][:, :T - 1])


# ---------------------------------------------------------------- 6. plugin and experiment
def _small_model(tmp_path, batch):
    from sketchformer_amd import dataloaders, models
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=%d,num_epochs=1,log_every=4" % batch,
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "sm")
    return model, dataset


def test_beam_search_rows_are_engine_rows_across_chunks(tmp_path):
    model, dataset = _small_model(tmp_path, 8)
    eng, tok = model.engine, dataset.tokenizer
    b = eng.get("output/bias").copy()
    b[tok.EOS] += 2.0
    eng.set("output/bias", b)
    x, _ = dataset.get_n_samples_from("valid", 5)                      # 5 sketches, 8 // 4 = 2 per call: three chunks
    z = model.predict_class(x)["embedding"]
    W, L = 4, dataset.hps["max_seq_len"] + 1
    res = model.beam_search_from_embedding(z, beam_width=W)
    assert res["recon"].shape == (5, W, L) and res["recon"].dtype == np.int32
    assert res["score"].shape == (5, W) and res["length"].shape == (5, W)
    for i in (0, 3, 4):                                               # alone in slot 0 of a call of its own
        t, s, ln = eng.beam_decode(np.concatenate([z[i:i + 1], np.zeros_like(z[:1])]), sos=tok.SOS, eos=tok.EOS, beam_width=W, n_valid=1)
        assert np.array_equal(s[0], res["score"][i]) and np.array_equal(ln[0], res["length"][i])
        for h in range(W):
            k = min(_first_eos(t[0, h], tok.EOS) + 1, t.shape[2])
            assert np.array_equal(res["recon"][i, h, :k], t[0, h, :k]) and (res["recon"][i, h, k:] == 0).all()
    same = model.beam_search(x, beam_width=W)
    assert np.array_equal(same["recon"], res["recon"]) and np.array_equal(same["score"], res["score"])
    one = model.beam_search(x, beam_width=1)                           # the greedy row and its log-likelihood
    greedy = model.predict(x)["recon"]
    for i in range(5):
        k = min(_first_eos(greedy[i], tok.EOS) + 1, greedy.shape[1])
        assert np.array_equal(one["recon"][i, 0, :k], greedy[i, :k])


def test_experiment_end_to_end(tmp_path, capsys):
    from sketchformer_amd import experiments
    model, dataset = _small_model(tmp_path, 8)
    Exp = experiments.get_experiment_by_name("beam-reconstructions")
    exp = Exp(Exp.parse_hparams("n_sketches=5,beam_width=3,length_alpha=0.5"), "b0", str(tmp_path))
    path = exp.compute(model)
    out = np.load(path, allow_pickle=True)
    L = dataset.hps["max_seq_len"]
    assert sorted(out.files) == sorted(["inputs", "labels", "greedy", "greedy_score", "beams", "scores", "lengths", "beam_width",
                                        "length_alpha"])
    assert out["inputs"].shape == (5, L) and out["labels"].shape == (5,)
    assert out["greedy"].shape == (5, L + 1) and out["greedy_score"].shape == (5,)
    assert out["beams"].shape == (5, 3, L + 1) and out["scores"].shape == (5, 3) and out["lengths"].shape == (5, 3)
    assert int(out["beam_width"]) == 3 and float(out["length_alpha"]) == np.float32(0.5)
    assert (out["beams"][:, :, 0] == dataset.tokenizer.SOS).all()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("beam-reconstructions:")]
    assert len(line) == 1 and "greedy" in line[0] and "best beam" in line[0]
