"""Teacher-forced scoring on the device (include/skf.h: skf_sequence_score; skf_score.hip).

The kernel is held to the float64 restatement of tests/score_reference.py on synthetic logits (float32 and bf16, aligned and
unaligned pitches, every edge rule of the header); the model-level calls are held to the float64 oracle's forward on the engine's own
parameters, and to the beam decoder's own scores.

The bound on one tok_logp is DERIVED, not measured: 16 * 2^-23 * max(1, max|z| over the row + ln V).  It covers one rounding of
z_y - m, a float32 sum of V exponentials from the fast exp (a few ulp each, relative about 1e-6 on a log of at most ln V), the log,
and one rounding of a result of magnitude at most max|z| + ln V: 7.5e-5 at |z| = 30."""
import functools

import numpy as np
import pytest
import torch

from oracle import sketchformer_oracle
import score_reference as ref
from test_gpu_decode_attention import SMALL, SMALL16, _build, _params

pytestmark = pytest.mark.gpu

NEG = -np.inf


# ---------------------------------------------------------------- synthetic cases (host only)
@functools.lru_cache(maxsize=None)
def make_case(B, T, V, seed=0):
    """(logits (B, T, V) float32, target (B, T) int64, eos): every kind of row and every kind of ending the header names.
    Sample b ends by b % 4: 0 neither EOS nor PAD, 1 EOS inside, 2 PADs without EOS, 3 EOS at t = 0.  Row (b, t) is of kind
    (b + t) % 8: 0, 1 randn * 3; 2 80 + randn; 3 -80 + randn; 4 the target's value again at a lower and at a higher index;
    5 a -inf target; 6 -inf non-targets; 7 a target outside [0, V) (-1 and V in turn)."""
    rng = np.random.RandomState(1000 * V + 10 * T + B + seed)
    eos = V - 1
    z = (rng.randn(B, T, V) * 3.0).astype(np.float32)
    y = rng.randint(1, max(V - 1, 2), size=(B, T)).astype(np.int64)            # neither PAD nor EOS
    for b in range(B):
        for t in range(T):
            kind = (b + t) % 8
            if kind == 2:
                z[b, t] = (80.0 + rng.randn(V)).astype(np.float32)
            elif kind == 3:
                z[b, t] = (-80.0 + rng.randn(V)).astype(np.float32)
            elif kind == 4:
                y[b, t] = min(max(y[b, t], 1), V - 2)                             # room on both sides
                z[b, t, rng.randint(0, y[b, t])] = z[b, t, y[b, t]]
                z[b, t, rng.randint(y[b, t] + 1, V)] = z[b, t, y[b, t]]
            elif kind == 5:
                z[b, t, y[b, t]] = NEG
            elif kind == 6:
                idx = rng.choice(V, size=max(V // 3, 1), replace=False)
                keep = z[b, t, y[b, t]]
                z[b, t, idx] = NEG
                z[b, t, y[b, t]] = keep                                          # the target (and so the maximum) stays finite
            elif kind == 7:
                y[b, t] = -1 if (b + t) % 16 == 7 else V
        end = b % 4
        if end == 1:
            y[b, T // 2] = eos
            y[b, T // 2 + 1:] = 0
        elif end == 2 and T > 1:
            y[b, (2 * T) // 3:] = 0
        elif end == 3:
            y[b, 0] = eos
    return z, y, eos


@functools.lru_cache(maxsize=None)
def expected(B, T, V, seed=0, bf16=False):
    """the restatement of a case, computed once"""
    z, y, eos = make_case(B, T, V, seed)
    if bf16:
        z = torch.from_numpy(z).to(torch.bfloat16).float().numpy()              # what the device widens, exactly
    return ref.sequence_score(z, y, eos), z


def _run(z, y, eos, ld=None, bf16=False, tgt_off=0, tgt_ld=None):
    """ops.sequence_score on device copies: logits in a buffer of row pitch ld, targets at column tgt_off of rows tgt_ld wide"""
    from sketchformer_amd import ops
    B, T, V = z.shape
    ld = V if ld is None else ld
    buf = torch.full((B * T, ld), 7.25, dtype=torch.float32)                     # (the pitch holds finite junk that must not count)
    buf[:, :V] = torch.from_numpy(z).reshape(B * T, V)
    buf = buf.to(torch.bfloat16 if bf16 else torch.float32).cuda()
    tgt_ld = tgt_off + T if tgt_ld is None else tgt_ld
    tg = torch.full((B, tgt_ld), 3, dtype=torch.int64)
    tg[:, tgt_off:tgt_off + T] = torch.from_numpy(y)
    logits = buf[:, :V] if ld != V else buf
    out = ops.sequence_score(logits.view(B, T, V) if ld == V else logits, tg.cuda(), eos, tgt_off=tgt_off, T=T)
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.float32, torch.int32]
    assert out[0].shape == (B, T) and out[1].shape == (B, T) and out[2].shape == (B,) and out[3].shape == (B,)
    return tuple(o.cpu().numpy() for o in out)


def _check(got, want, z, V, name=""):
    lp, rk, s, n = got
    (wlp, wrk, ws, wn) = want
    B, T = wlp.shape
    assert np.array_equal(n, wn), (name, n, wn)
    assert np.array_equal(rk, wrk), (name, np.argwhere(rk != wrk)[:5])
    worst = 0.0
    for b in range(B):
        for t in range(T):
            if t >= wn[b]:
                assert lp[b, t] == 0.0 and not np.signbit(lp[b, t]) and rk[b, t] == -1, (name, b, t)
            elif not np.isfinite(wlp[b, t]):
                assert lp[b, t] == wlp[b, t], (name, b, t, lp[b, t], wlp[b, t])     # the same infinity
            else:
                bound = ref.logp_bound(z[b, t], V)
                err = abs(float(lp[b, t]) - wlp[b, t])
                worst = max(worst, err / bound)
                assert err <= bound, (name, b, t, lp[b, t], wlp[b, t], err, bound)
        assert s[b].tobytes() == ref.sequential_sum_f32(lp[b], n[b]).tobytes(), (name, b, s[b])
    print("%s: worst tok_logp error %.3f of its bound" % (name, worst))


# ---------------------------------------------------------------- a. the kernel against the restatement, float32
SHAPES = [(V, B, T) for V in (5, 52, 53, 1003, 1004) for (B, T) in ((1, 1), (5, 23), (3, 199))] + [(10004, 2, 5)]


@pytest.mark.parametrize("V,B,T", SHAPES)
def test_kernel_follows_the_rule_f32(V, B, T):
    z, y, eos = make_case(B, T, V)
    want, _ = expected(B, T, V)
    _check(_run(z, y, eos), want, z, V, "V=%d B=%d T=%d" % (V, B, T))


@pytest.mark.parametrize("extra", [3, 4], ids=["ld=V+3", "ld=V+4"])
def test_kernel_row_pitch_f32(extra):
    """a pitch that breaks the 16-byte alignment of the rows (element-wise path at V % 4 == 0) and one that keeps it"""
    B, T, V = 5, 23, 1004
    z, y, eos = make_case(B, T, V)
    want, _ = expected(B, T, V)
    _check(_run(z, y, eos, ld=V + extra), want, z, V, "ld=V+%d" % extra)


def test_kernel_target_offset_and_pitch():
    B, T, V = 5, 23, 52
    z, y, eos = make_case(B, T, V)
    want, _ = expected(B, T, V)
    _check(_run(z, y, eos, tgt_off=1, tgt_ld=T + 6), want, z, V, "tgt_off=1")


# ---------------------------------------------------------------- b. the same on bf16 logits
@pytest.mark.parametrize("pitched", [False, True], ids=["ld=V", "ld=pad8(V)"])
@pytest.mark.parametrize("B,T", [(1, 1), (5, 23), (3, 199)])
@pytest.mark.parametrize("V", [52, 1004])
def test_kernel_follows_the_rule_bf16(V, B, T, pitched):
    """ld = pad8(V) is the pitch of the bf16 model's buffers (16-byte rows: the vector path); ld = V takes the element-wise one"""
    z, y, eos = make_case(B, T, V)
    want, zw = expected(B, T, V, bf16=True)
    ld = (V + 7) // 8 * 8 if pitched else V
    _check(_run(z, y, eos, ld=ld, bf16=True), want, zw, V, "bf16 V=%d B=%d T=%d ld=%d" % (V, B, T, ld))


# ---------------------------------------------------------------- c. skipped rows are not read
@pytest.mark.parametrize("V,bf16", [(1004, False), (53, False), (10004, False), (1004, True)])
def test_rows_behind_the_end_are_not_read(V, bf16):
    B, T = (2, 5) if V == 10004 else (5, 23)
    z, y, eos = make_case(B, T, V, seed=1)
    n = [ref.scored_length(y[b], eos) for b in range(B)]
    assert min(n) < T                                                         # there is something to skip
    clean = _run(z, y, eos, bf16=bf16)
    zd, yd = z.copy(), y.copy()
    for b in range(B):
        zd[b, n[b]:] = np.nan
        if n[b] > 0 and y[b, n[b] - 1] == eos:                                # behind an EOS anything goes, terminators included
            yd[b, n[b]:] = np.array([-9, 10 ** 12, 0, eos, V + 3] * T)[:T - n[b]]
        elif n[b] < T:                                                        # behind the first PAD: anything but an EOS
            yd[b, n[b] + 1:] = np.array([10 ** 12, -5, 0, V + 3] * T)[:T - n[b] - 1]
    assert [ref.scored_length(yd[b], eos) for b in range(B)] == n
    dirty = _run(zd, yd, eos, bf16=bf16)
    for a, c in zip(clean, dirty):
        assert a.tobytes() == c.tobytes()


# ---------------------------------------------------------------- d. isolation and determinism
@pytest.mark.parametrize("V", [53, 1004, 10004])
def test_isolation_and_determinism(V):
    T = 5 if V == 10004 else 23
    z, y, eos = make_case(5, T, V, seed=2)
    z2, y2, _ = make_case(5, T, V, seed=3)
    src = 1                                                                   # the sample with an EOS inside
    alone = _run(z[src:src + 1], y[src:src + 1], eos)
    first = _run(np.concatenate([z[src:src + 1], z[:4]]), np.concatenate([y[src:src + 1], y[:4]]), eos)
    last = _run(np.concatenate([z2[:4], z[src:src + 1]]), np.concatenate([y2[:4], y[src:src + 1]]), eos)
    for k in range(4):
        assert alone[k][0].tobytes() == first[k][0].tobytes() == last[k][4].tobytes(), k
    again = _run(np.concatenate([z2[:4], z[src:src + 1]]), np.concatenate([y2[:4], y[src:src + 1]]), eos)
    for a, c in zip(last, again):
        assert a.tobytes() == c.tobytes()


# ---------------------------------------------------------------- e. model level, fp32
def _sos_eos(ocfg):
    return ocfg.vocab_size - 2, ocfg.vocab_size - 1


def _batch(ocfg, B, seed):
    from sketchformer_amd import synthetic
    x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=seed)
    x[0, 7:] = 0                                                              # a row that ends on a PAD, without EOS
    x[1, 3:] = 0
    return x


@pytest.mark.parametrize("B", [6, 8])
@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_engine_score_against_the_oracle(blind, B):
    from sketchformer_amd import ops
    eng, ocfg = _build(B, blind=blind)
    sos, eos = _sos_eos(ocfg)
    x = _batch(ocfg, B, seed=8)
    T = ocfg.seq_len - 1
    lp, rk, s, n = (t.cpu().numpy() for t in eng.score(x, eos=eos))
    assert lp.shape == (B, T) and rk.shape == (B, T) and s.shape == (B,) and n.shape == (B,)
    out, _ = sketchformer_oracle.forward(_params(eng), ocfg, x, x[:, :-1], training=False)
    wlp, _, ws, wn = ref.sequence_score(out["recon"], x[:, 1:], eos)
    assert np.array_equal(n, wn) and n.min() < T and n.max() > 3, n
    assert np.abs(lp - wlp).max() <= 2e-4, np.abs(lp - wlp).max()
    assert (np.abs(s - ws) <= 2e-4 * n).all(), (s, ws, n)
    for b in range(B):
        assert s[b].tobytes() == ref.sequential_sum_f32(lp[b], n[b]).tobytes()
    # ranks: exact against the device's own logits (against the oracle's, near-ties would decide)
    dev_logits = eng.buffer("logits")
    assert dev_logits.dtype == torch.float32
    _, drk, _, _ = ref.sequence_score(dev_logits.cpu().numpy().reshape(B, T, -1), x[:, 1:], eos)
    assert np.array_equal(rk, drk)
    assert (rk[:, 0] >= 0).all()
    # the op on the engine's pitched view gives the same bits
    again = ops.sequence_score(dev_logits, torch.from_numpy(x).cuda(), eos, tgt_off=1, T=T)
    for a, c in zip((lp, rk, s, n), again):
        assert a.tobytes() == c.cpu().numpy().tobytes()
    # n_valid cuts the rows; a target of its own: the same as scoring the input against itself
    part = eng.score(x, x.copy(), n_valid=3, eos=eos)
    assert part[0].shape == (3, T) and part[2].shape == (3,)
    for a, c in zip((lp, rk, s, n), part):
        assert a[:3].tobytes() == c.cpu().numpy().tobytes()
    print("blind=%s B=%d: worst tok_logp error %.3g, worst seq_logp error per position %.3g"
          % (blind, B, np.abs(lp - wlp).max(), (np.abs(s - ws) / np.maximum(n, 1)).max()))


# ---------------------------------------------------------------- f. model level, bf16
def test_engine_score_bf16_model():
    B = 6
    eng, ocfg = _build(B, blind=True, act_dtype="bf16", **SMALL16)
    sos, eos = _sos_eos(ocfg)
    x = _batch(ocfg, B, seed=8)
    T, V = ocfg.seq_len - 1, ocfg.vocab_size
    got = tuple(t.cpu().numpy() for t in eng.score(x, eos=eos))
    dev_logits = eng.buffer("logits")
    assert dev_logits.dtype == torch.bfloat16 and dev_logits.stride(0) % 8 == 0
    z = dev_logits.float().cpu().numpy().reshape(B, T, V)
    _check(got, ref.sequence_score(z, x[:, 1:], eos), z, V, "bf16 model")
    assert got[3].min() < T and got[3].max() > 3


# ---------------------------------------------------------------- h. errors
def test_errors():
    from sketchformer_amd import engine, ops
    eng, ocfg = _build(4, continuous=True)
    with pytest.raises(ValueError, match="token models"):
        eng.score(np.zeros((4, ocfg.seq_len, 5), np.float32))
    eng = engine.TrainEngine(engine.make_config(batch=4, dropout_rate=0.0, use_graph=False, do_reconstruction=False, **SMALL), init_seed=1)
    with pytest.raises(ValueError, match="do_reconstruction"):
        eng.score(np.ones((4, SMALL["seq_len"]), np.int64))
    z = torch.zeros(2, 3, 8, device="cuda")
    y = torch.ones(2, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="logits"):
        ops.sequence_score(z.double(), y, 7)
    with pytest.raises(ValueError, match="logits"):
        ops.sequence_score(z.half(), y, 7)
    with pytest.raises(ValueError, match="target"):
        ops.sequence_score(z, y[:, :2], 7)                                   # too narrow
    with pytest.raises(ValueError, match="target"):
        ops.sequence_score(z, y, 7, tgt_off=1)
    with pytest.raises(ValueError, match="target"):
        ops.sequence_score(z, y.int(), 7)
    with pytest.raises(ValueError, match="T"):
        ops.sequence_score(z.view(6, 8), y, 7)                               # (B * T, V) without T
    eng, ocfg = _build(4)
    with pytest.raises(ValueError, match="tar"):
        eng.score(np.ones((4, ocfg.seq_len), np.int64), np.ones((4, ocfg.seq_len - 1), np.int64))


# ---------------------------------------------------------------- g. beam consistency
BEAM_BATCH = (12, 3)      # synthetic.token_batch(8, ..., seed=12), row 3


def test_beam_scores_are_teacher_forced_scores():
    """The beam decoder's sum of log p and its length, recomputed by the forward and the scoring kernel.  Both sides are within
    2e-4 * length of the oracle by existing bars (test_gpu_beam.py; (e) above), hence 4e-4 * length of each other.

    How BEAM_BATCH was picked: on the CPU, from the oracle search of test_gpu_beam.py (`oracle_search` on the engine's parameters
    rebuilt on the host: engine.keras_init(seed 1) plus the bias / LayerNorm draws of `_build`, the output bias nudged).  Under
    PAD_NUDGE every hypothesis holds PADs, and one WITHOUT an EOS is by the rule scored to its first PAD only, so seq_len == length
    can hold for EOS-terminated hypotheses alone: the sketch was searched (seeds 0 .. 479, rows 0 .. 7) for four hypotheses that
    all end in EOS, at least one early and one at position MAX_STEPS exactly, with an oracle margin >= 4e-4 * MAX_STEPS.  (12, 3)
    is the first hit: lengths 7, 8, 11, 12, margin 5.05e-3."""
    from sketchformer_amd import synthetic
    from test_gpu_beam import EOS_NUDGE, MAX_STEPS, PAD_NUDGE, nudge
    assert (PAD_NUDGE, EOS_NUDGE, MAX_STEPS) == (3.0, 2.0, 12)
    B = W = 4
    eng, ocfg = _build(B, blind=True)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    L = ocfg.seq_len
    seed, row = BEAM_BATCH
    x8, _ = synthetic.token_batch(8, L, ocfg.vocab_size, ocfg.n_classes, seed=seed)
    xb = x8[[row, 0, 1, 2]]
    eng.encode(xb)
    emb = eng.buffer("embedding").float()[:1].clone()
    tok, score, length = eng.beam_decode(emb, sos=sos, eos=eos, max_steps=MAX_STEPS, beam_width=W)
    assert tok.shape[:2] == (1, W) and tok.shape[2] <= MAX_STEPS + 1
    tar = np.zeros((B, L), np.int64)
    tar[:, :tok.shape[2]] = tok[0]
    lp, rk, s, n = (t.cpu().numpy() for t in eng.score(np.repeat(xb[:1], W, axis=0), tar, eos=eos))
    early = full = 0
    for k in range(W):
        print("hypothesis %d: length %d, beam score %.6f, teacher-forced %.6f (scored length %d)" % (k, length[0, k], score[0, k], s[k], n[k]))
        early += int(length[0, k] < MAX_STEPS)
        full += int(length[0, k] == MAX_STEPS)
    for k in range(W):
        assert n[k] == length[0, k], (k, n[k], length[0, k], tok[0, k])
        assert abs(float(s[k]) - float(score[0, k])) <= 4e-4 * length[0, k], (k, s[k], score[0, k], length[0, k])
    assert early >= 1 and full >= 1, (early, full, length)


# ---------------------------------------------------------------- i. plugin and experiment
def _small_model(tmp_path, batch):
    from test_gpu_beam import _small_model as build
    return build(tmp_path, batch)


def test_model_score_rows_are_engine_rows_across_chunks(tmp_path):
    model, dataset = _small_model(tmp_path, 4)
    eng, tok = model.engine, dataset.tokenizer
    L, B = dataset.hps["max_seq_len"], 4
    n = 2 * B + 3
    x, _ = dataset.get_n_samples_from("valid", n)
    x = np.asarray(x)[:n].reshape(n, L)
    res = model.score(x)
    assert res["logp"].shape == (n,) and res["length"].shape == (n,) and res["token_logp"].shape == (n, L - 1)
    assert res["rank"].shape == (n, L - 1) and res["perplexity"].shape == (n,) and res["complete"].shape == (n,)
    assert res["logp"].dtype == np.float32 and res["length"].dtype == np.int32 and res["rank"].dtype == np.int32
    pad = np.zeros((B, L), np.int64)
    for i in range(0, n, B):                                                  # chunk by chunk: the engine's own rows
        m = min(B, n - i)
        pad[:] = 0
        pad[:m] = x[i:i + m]
        lp, rk, s, ln = (t.cpu().numpy() for t in eng.score(pad, n_valid=m, eos=tok.EOS))
        assert res["token_logp"][i:i + m].tobytes() == lp.tobytes() and res["rank"][i:i + m].tobytes() == rk.tobytes()
        assert res["logp"][i:i + m].tobytes() == s.tobytes() and res["length"][i:i + m].tobytes() == ln.tobytes()
    # a row's result does not depend on its chunk: row 5 (slot 1 of the second chunk) alone, and in another slot among others
    one = model.score(x[5])
    other = model.score(x[[9, 2, 5]])
    for k in res:
        assert np.array_equal(one[k][0], res[k][5]) and np.array_equal(other[k][2], res[k][5]), k
    assert np.allclose(res["perplexity"], np.exp(-res["logp"].astype(np.float64) / np.maximum(res["length"], 1)), rtol=1e-12)
    # seq_len + 1 columns with the EOS in the last one: outside the window, scored on the seq_len - 1 positions that fit
    tar = np.full((2, L + 1), 5, np.int64)
    tar[:, 0] = tok.SOS
    tar[0, L] = tok.EOS
    tar[1, 4] = tok.EOS
    tar[1, 5:] = 0
    r2 = model.score(x[:2], tar)
    assert r2["complete"].tolist() == [False, True] and r2["length"].tolist() == [L - 1, 4]
    assert (r2["rank"][0] >= 0).all() and np.isfinite(r2["logp"]).all()
    greedy = model.predict(x[:3])["recon"]                                    # an untrained model's greedy rows: scoring them must not raise
    r3 = model.score(x[:3], greedy)
    assert r3["logp"].shape == (3,) and np.isfinite(r3["logp"]).all()


def test_experiment_end_to_end(tmp_path, capsys):
    from sketchformer_amd import experiments
    model, dataset = _small_model(tmp_path, 8)
    eng, tok = model.engine, dataset.tokenizer
    b = eng.get("output/bias").copy()
    b[tok.EOS] += 6.0                             # hypotheses end in an EOS: the beam's length is the scored length (see (g))
    eng.set("output/bias", b)
    Exp = experiments.get_experiment_by_name("reconstruction-likelihood")
    assert Exp.requires_model
    exp = Exp(Exp.parse_hparams("n_sketches=8,n_samples=3,beam_width=2"), "r0", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    L = dataset.hps["max_seq_len"]
    assert sorted(out.files) == sorted([
        "inputs", "labels", "logp", "length", "perplexity", "complete", "corpus_perplexity", "top1_accuracy", "topk_accuracy", "top_k",
        "classes", "class_nll", "worst", "samples", "sample_logp", "sample_length", "greedy", "greedy_logp", "temperature", "top_p",
        "seed", "beams", "beam_score", "beam_length", "beam_logp", "beam_scored_length"])
    assert out["inputs"].shape == (8, L) and out["logp"].shape == (8,) and out["length"].shape == (8,) and out["perplexity"].shape == (8,)
    logp, length = out["logp"].astype(np.float64), out["length"].astype(np.int64)
    assert float(out["corpus_perplexity"]) == pytest.approx(np.exp(-logp.sum() / length.sum()), rel=1e-12)
    assert 0.0 <= float(out["top1_accuracy"]) <= float(out["topk_accuracy"]) <= 1.0 and int(out["top_k"]) == 5
    assert len(out["classes"]) == len(out["class_nll"]) and set(out["classes"]) == set(out["labels"])
    nll = -logp / np.maximum(length, 1)
    assert out["worst"].shape == (8,) and sorted(out["worst"]) == list(range(8)) and (np.diff(nll[out["worst"]]) <= 0).all()
    assert out["samples"].shape == (8, 3, L + 1) and out["sample_logp"].shape == (8, 3) and out["greedy_logp"].shape == (8,)
    assert (np.diff(out["sample_logp"], axis=1) <= 0).all()                   # best first
    assert out["beams"].shape == (8, 2, L + 1) and out["beam_score"].shape == (8, 2) and out["beam_logp"].shape == (8, 2)
    assert np.array_equal(out["beam_scored_length"], out["beam_length"])
    assert (np.abs(out["beam_logp"].astype(np.float64) - out["beam_score"]) <= 4e-4 * out["beam_length"]).all()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("reconstruction-likelihood:")]
    assert len(line) == 1 and "corpus perplexity" in line[0] and "top-5 accuracy" in line[0]
    # a continuous model is refused
    class _Continuous:
        class dataset:
            hps = {"use_continuous_data": True}
    with pytest.raises(ValueError, match="token models"):
        Exp(Exp.parse_hparams("n_sketches=2"), "r1", str(tmp_path)).compute(_Continuous())
