"""Sketch completion on the device: prefix-forced decoding with a cache prefill (include/skf.h: the rule).

Forced columns must equal the prefix, free positions must follow the float64 oracle, and the prefill (the cache rows of all forced
positions in num_layers launches) must give the bits that stepping through the prefix gives: outputs, column counts and the K|V
cache rows of every layer.  Beam scores are held to the bar of tests/test_gpu_beam.py, 2e-4 per scored position."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_reference
import completion_reference as cref
import sampling_reference as sref
from test_gpu_decode_attention import CFG2, SMALL, SMALL16, _build, _inputs, _params
from test_gpu_sampling import _stop_columns, _teacher_forced_logits

pytestmark = pytest.mark.gpu

MAX_STEPS = 24
AMBIGUOUS_CAP = 0.05
GREEDY = (1.0, 1, 1.0)                    # greedy as a selection rule: the arg-max alone survives
CASES = {"small": dict(SMALL), "dh32": dict(SMALL, d_model=64, num_heads=2), "small16": dict(SMALL16),
         "small16_bf16": dict(SMALL16, act_dtype="bf16")}
RAGGED = (0, 1, 5, 23)
WHOLE = (24, 24, 24, 24)
SAMPLING = dict(temperature=1.1, top_k=20, top_p=0.95, seed=5, stream_ids=[11, 5, 40, 2])


def _sos_eos(ocfg):
    return ocfg.vocab_size - 2, ocfg.vocab_size - 1


@functools.lru_cache(maxsize=None)
def _shared(case, blind, B=4):
    """(engine, oracle config, embedding, lengths) of one case; shared by the tests that leave the parameters alone"""
    eng, ocfg = _build(B, blind=blind, **CASES[case])
    emb, tlen = _inputs(eng, ocfg, B, seed=8)
    return eng, ocfg, emb, tlen


def _caches(eng, ocfg, B):
    """the self-attention K|V rows of the last decode as raw bits: [layer] (B, L, 2 d) int32"""
    return [eng.buffer("decode/cache%d" % l).contiguous().view(torch.int32).cpu().numpy().reshape(B, ocfg.seq_len, 2 * ocfg.d_model)
            for l in range(ocfg.num_layers)]


def _poison_caches(eng, num_layers):
    """NaN into every K|V cache row: nothing clears the caches between decodes, so without this a decode that fails to write a
    row would find the row an earlier decode of the same inputs left there - in the comparison and in its own attention"""
    for l in range(num_layers):
        eng.buffer("decode/cache%d" % l).fill_(float("nan"))


def _decode(eng, ocfg, emb, el, prefix, lens, prefill, sampled=False):
    sos, eos = _sos_eos(ocfg)
    _poison_caches(eng, ocfg.num_layers)
    kw = dict(expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS, prefix=prefix, prefix_len=lens, prefill=prefill)
    out = eng.sample_decode(emb, **SAMPLING, **kw) if sampled else eng.greedy_decode(emb, **kw)
    return out, _caches(eng, ocfg, emb.shape[0])


def _assert_prefill_equals_stepping(eng, ocfg, emb, el, prefix, lens, sampled=False):
    """outputs, column counts and cache rows s < len[b] of every layer, as raw bits; returns the stepwise output"""
    step, c_step = _decode(eng, ocfg, emb, el, prefix, lens, False, sampled)
    fill, c_fill = _decode(eng, ocfg, emb, el, prefix, lens, True, sampled)
    assert step.shape == fill.shape and np.array_equal(step, fill), (step, fill)
    for l in range(ocfg.num_layers):
        for b, n in enumerate(lens):
            assert not np.isnan(c_fill[l][b, :n].view(np.float32)).any(), ("layer %d row %d: a prefix cache row was not written" % (l, b))
            same = (c_step[l][b, :n] == c_fill[l][b, :n]).all(axis=1)
            assert same.all(), ("layer %d row %d: cache rows %s differ" % (l, b, np.nonzero(~same)[0].tolist()))
    return step


def _modes(case):
    return ("blind", "nonblind", "nonblind_nolen") if case == "small" else ("blind", "nonblind")


def _mode(case, mode):
    eng, ocfg, emb, tlen = _shared(case, mode == "blind")
    return eng, ocfg, emb, (tlen if mode == "nonblind" else None)


CASE_MODES = [(c, m) for c in CASES for m in _modes(c)]


# ---------------------------------------------------------------- 1. no prefix
@pytest.mark.parametrize("case", list(CASES))
def test_empty_prefix_is_the_plain_decode(case):
    eng, ocfg, emb, _ = _shared(case, True)
    sos, eos = _sos_eos(ocfg)
    kw = dict(sos=sos, eos=eos, max_steps=MAX_STEPS)
    greedy = eng.greedy_decode(emb, **kw)
    sampled = eng.sample_decode(emb, **SAMPLING, **kw)
    none = np.zeros((4, 1), np.int64)
    for prefill in (True, False):
        pk = dict(prefix=none, prefix_len=[0, 0, 0, 0], prefill=prefill)
        got = eng.greedy_decode(emb, **kw, **pk)
        assert got.dtype == greedy.dtype and got.shape == greedy.shape and np.array_equal(got, greedy)
        got = eng.sample_decode(emb, **SAMPLING, **kw, **pk)
        assert got.shape == sampled.shape and np.array_equal(got, sampled)


# ---------------------------------------------------------------- 2. forced columns and self-consistency
@pytest.mark.parametrize("case,mode", CASE_MODES)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_own_output_as_prefix_reproduces_it(case, mode, sampled):
    """The device's own sequence G, cut at ragged lengths and forced whole: the decode gives G again, columns and column count
    included, with the prefill and without.  Sampled: same seed and stream ids - a position keeps its uniform."""
    eng, ocfg, emb, el = _mode(case, mode)
    sos, eos = _sos_eos(ocfg)
    kw = dict(expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS)
    G = eng.sample_decode(emb, **SAMPLING, **kw) if sampled else eng.greedy_decode(emb, **kw)
    for lens in (RAGGED, WHOLE):
        lens = [min(n, G.shape[1] - 1) for n in lens]             # (G ends early when every row has drawn its EOS)
        for prefill in (False, True):
            got, _ = _decode(eng, ocfg, emb, el, G[:, 1:], lens, prefill, sampled)
            assert got.shape == G.shape and np.array_equal(got, G), (lens, prefill, got, G)


# ---------------------------------------------------------------- 3. foreign prefix against the oracle
FOREIGN_LENS = (9, 12, 0, 15)


def foreign_case(blind, vocab=SMALL["vocab_size"], d_model=SMALL["d_model"], seq_len=SMALL["seq_len"]):
    """Host-made inputs of the oracle case: (embedding, expected_len, prefix, lengths).  Random tokens; row 0 holds a PAD inside
    its prefix, row 1 an EOS (its prefix goes on behind it), row 2 has no prefix at all."""
    rng = np.random.RandomState(300 + (0 if blind else 1))
    emb = (rng.randn(4, d_model) * 0.5).astype(np.float32)        # attn_version 1: the embedding has d_model columns
    el = None if blind else rng.randint(3, seq_len, size=4).astype(np.int32)
    prefix = rng.randint(1, vocab - 3, size=(4, max(FOREIGN_LENS))).astype(np.int64)
    prefix[0, 4] = 0
    prefix[1, 6] = vocab - 1
    return emb, el, prefix, list(FOREIGN_LENS)


def nudge(bias, eos):
    """PADs and early ends occur, as in tests/test_gpu_sampling.py"""
    b = np.array(bias, copy=True)
    b[0] += 3.0
    b[eos] += 2.0
    return b


@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_foreign_prefix_follows_the_oracle(blind):
    eng, ocfg = _build(4, blind=blind)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    P = _params(eng)
    emb, el, prefix, lens = foreign_case(blind)
    recon = _assert_prefill_equals_stepping(eng, ocfg, emb, el, prefix, lens)          # (4. for this case)
    assert (recon[:, 0] == sos).all()
    ncols = recon.shape[1]
    assert ncols == _stop_columns(recon, eos, MAX_STEPS)
    logits = _teacher_forced_logits(P, ocfg, emb, recon.astype(np.int64), el)
    free = skipped = 0
    for b in range(4):
        n = min(lens[b], ncols - 1)
        assert np.array_equal(recon[b, 1:1 + n], prefix[b, :n])                        # forced columns are the prefix
        for i in range(lens[b], ncols - 1):
            free += 1
            if sref.ambiguous(logits[b, i], GREEDY):
                skipped += 1
                continue
            assert sref.accepts(logits[b, i], GREEDY, 0.5, recon[b, i + 1]), (b, i, int(recon[b, i + 1]), int(np.argmax(logits[b, i])))
    assert free >= 20 and skipped <= AMBIGUOUS_CAP * free, (skipped, free)
    # the oracle's own forced-greedy run (tests/completion_reference.py) on the same inputs: it stays under the cap as well, and
    # up to its first ambiguous position the device took every step it took - forced and free tokens, and the column count
    amb = []

    def logits_fn(tokens):
        return _teacher_forced_logits(P, ocfg, emb, np.concatenate([tokens, np.zeros((4, 1), np.int64)], axis=1), el)[:, -1]
    want, forced = cref.forced_greedy(logits_fn, prefix, lens, sos, eos, MAX_STEPS, ocfg.vocab_size,
                                      on_free=lambda b, s, row, tok: amb.append(s) if sref.ambiguous(row, GREEDY) else None)
    n_free = int((~forced[:, 1:]).sum())
    assert len(amb) <= AMBIGUOUS_CAP * n_free, (len(amb), n_free)
    sure = min(amb) + 1 if amb else want.shape[1]                 # columns decided without an ambiguous step
    assert np.array_equal(recon[:, :sure], want[:, :sure]) and (amb or recon.shape == want.shape), (recon, want)
    for b in range(4):
        assert forced[b, 1:].tolist() == [s < lens[b] for s in range(want.shape[1] - 1)]
    print("free positions %d, ambiguous %d, columns %d" % (free, skipped, ncols))


# ---------------------------------------------------------------- 4. prefill equals stepping, bit for bit
@pytest.mark.parametrize("case,mode", CASE_MODES)
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_prefill_equals_stepping_bit_for_bit(case, mode, sampled):
    eng, ocfg, emb, el = _mode(case, mode)
    sos, eos = _sos_eos(ocfg)
    kw = dict(expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS)
    G = eng.sample_decode(emb, **SAMPLING, **kw) if sampled else eng.greedy_decode(emb, **kw)
    for lens in (RAGGED, WHOLE):
        lens = [min(n, G.shape[1] - 1) for n in lens]
        _assert_prefill_equals_stepping(eng, ocfg, emb, el, G[:, 1:], lens, sampled)
    # a prefix the model would not have chosen: every layer's rows depend on it
    rng = np.random.RandomState(17)
    foreign = rng.randint(1, ocfg.vocab_size - 3, size=(4, MAX_STEPS)).astype(np.int64)
    foreign[1, 3] = 0
    _assert_prefill_equals_stepping(eng, ocfg, emb, el, foreign, [7, 20, 2, 13], sampled)


def test_prefill_equals_stepping_at_cfg2_dimensions():
    """d = 128: attend goes from one pass over the keys to two at 129 keys, which no small case reaches"""
    from sketchformer_amd import engine, synthetic
    B = 4
    eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.0, use_graph=False, seed=1, **CFG2), init_seed=2)
    x, _ = synthetic.token_batch(B, CFG2["seq_len"], CFG2["vocab_size"], CFG2["n_classes"], seed=0)
    eng.encode(x)
    eng.synchronize()
    emb = eng.buffer("embedding").float().cpu().numpy()
    V, L, N, d = CFG2["vocab_size"], CFG2["seq_len"], CFG2["num_layers"], CFG2["d_model"]
    rng = np.random.RandomState(5)
    prefix = rng.randint(1, V - 3, size=(B, L)).astype(np.int64)
    prefix[2, 40] = 0
    lens = [128, 129, 150, 199]
    res = []
    for prefill in (False, True):
        _poison_caches(eng, N)
        out = eng.greedy_decode(emb, sos=V - 2, eos=V - 1, prefix=prefix, prefix_len=lens, prefill=prefill)
        res.append((out, [eng.buffer("decode/cache%d" % l).contiguous().view(torch.int32).cpu().numpy().reshape(B, L, 2 * d)
                          for l in range(N)]))
    (step, c_step), (fill, c_fill) = res
    assert step.shape == fill.shape and np.array_equal(step, fill)
    for b in range(B):
        assert np.array_equal(step[b, 1:1 + lens[b]], prefix[b, :lens[b]])
        for l in range(N):
            assert not np.isnan(c_fill[l][b, :lens[b]].view(np.float32)).any(), (l, b)
            same = (c_step[l][b, :lens[b]] == c_fill[l][b, :lens[b]]).all(axis=1)
            assert same.all(), (l, b, np.nonzero(~same)[0].tolist())


# ---------------------------------------------------------------- 5. stop inside the prefix
def _raw_prefix_decode(eng, ocfg, emb, prefix, lens, stepwise, fill=-7):
    """the C entry on a caller buffer filled with `fill`: (buffer (B, MAX_STEPS + 1), reported columns)"""
    from sketchformer_amd import _lib
    B = emb.shape[0]
    sos, eos = _sos_eos(ocfg)
    e = torch.from_numpy(emb).cuda()
    tok = torch.from_numpy(np.ascontiguousarray(prefix)).cuda()
    out = torch.full((B, MAX_STEPS + 1), fill, dtype=torch.int64, device="cuda")
    arr = (C.c_int * B)(*lens)
    pf = _lib.SkfPrefix(tokens=tok.data_ptr(), ld=tok.shape[1], len_host=arr, stepwise=stepwise)
    n_out = C.c_int(0)
    torch.cuda.synchronize()
    _lib.call("skf_model_prefix_decode", eng.handle, C.c_void_p(e.data_ptr()), None, B, sos, eos, MAX_STEPS, C.c_void_p(out.data_ptr()),
              C.byref(n_out), C.byref(pf), None, None, C.c_void_p(eng.stream.cuda_stream))
    eng.synchronize()
    return out.cpu().numpy(), n_out.value


@pytest.mark.parametrize("case", ["small", "small16_bf16"])
def test_decode_ends_inside_the_prefix(case):
    eng, ocfg, emb, _ = _shared(case, True)
    sos, eos = _sos_eos(ocfg)
    rng = np.random.RandomState(3)
    prefix = rng.randint(1, ocfg.vocab_size - 3, size=(4, 12)).astype(np.int64)
    lens = [5, 9, 4, 12]
    for b, col in enumerate((3, 7, 2, 5)):                        # every row's prefix holds an EOS, at these output columns
        prefix[b, col - 1] = eos
    for prefill in (True, False):
        got = eng.greedy_decode(emb, sos=sos, eos=eos, max_steps=MAX_STEPS, prefix=prefix, prefix_len=lens, prefill=prefill)
        assert got.shape == (4, 8), (prefill, got.shape)
        for b in range(4):
            n = min(lens[b], 7)
            assert np.array_equal(got[b, 1:1 + n], prefix[b, :n])
        raw, ncols = _raw_prefix_decode(eng, ocfg, emb, prefix, lens, 0 if prefill else 1)
        assert ncols == 8 and np.array_equal(raw[:, :8], got) and (raw[:, 8:] == -7).all()      # nothing behind them is written
    # the stop test counts the first n_valid rows alone
    got = eng.greedy_decode(emb, n_valid=1, sos=sos, eos=eos, max_steps=MAX_STEPS, prefix=prefix, prefix_len=lens)
    assert got.shape == (1, 4)


# ---------------------------------------------------------------- 6. beams
@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_beam_width_one_with_a_prefix_is_greedy_with_it(blind):
    B = 8
    eng, ocfg, emb, tlen = _shared("small", blind, B)
    el = None if blind else tlen
    sos, eos = _sos_eos(ocfg)
    rng = np.random.RandomState(23)
    prefix = rng.randint(1, ocfg.vocab_size - 3, size=(B, 10)).astype(np.int64)
    lens = [0, 1, 5, 10, 3, 7, 2, 9]
    kw = dict(expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS, prefix=prefix, prefix_len=lens)
    want = eng.greedy_decode(emb, **kw)
    tok, score, length = eng.beam_complete(emb, beam_width=1, **kw)
    assert tok.shape == (B, 1, want.shape[1]) and np.array_equal(tok[:, 0], want)


@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
def test_beam_search_continues_the_prefix(blind):
    B, W = 8, 4
    n = B // W
    eng, ocfg = _build(B, blind=blind)
    sos, eos = _sos_eos(ocfg)
    eng.set("output/bias", nudge(eng.get("output/bias"), eos))
    P = _params(eng)
    rng = np.random.RandomState(41 + int(blind))
    emb = (rng.randn(n, SMALL["d_model"]) * 0.5).astype(np.float32)
    el = None if blind else rng.randint(3, SMALL["seq_len"], size=n).astype(np.int32)
    prefix = rng.randint(1, ocfg.vocab_size - 3, size=(n, 8)).astype(np.int64)
    prefix[1, 2] = 0                                              # a PAD inside the second sketch's prefix
    lens = [3, 6]
    tok, score, length = eng.beam_complete(emb, prefix, lens, expected_len=el, sos=sos, eos=eos, max_steps=MAX_STEPS, beam_width=W)
    T = tok.shape[2]
    assert tok.shape == (n, W, T) and (tok[:, :, 0] == sos).all()
    worst = 0.0
    for g in range(n):
        p = lens[g]
        assert (tok[g, :, 1:1 + p] == prefix[g, :p]).all()        # every hypothesis starts with its sketch's prefix
        assert (np.diff(score[g]) <= 0).all() and np.isfinite(score[g]).all()
        assert len(set(tuple(int(v) for v in tok[g, k]) for k in range(W))) == W
        e = np.repeat(emb[g:g + 1], W, axis=0)
        lg = _teacher_forced_logits(P, ocfg, e, np.concatenate([tok[g], np.zeros((W, 1), tok.dtype)], axis=1).astype(np.int64),
                                    None if el is None else np.repeat(el[g], W))
        for k in range(W):
            ln = int(length[g, k])
            n_free = ln - p
            assert n_free >= 1
            want = sum(beam_reference.log_softmax(lg[k, i])[tok[g, k, i + 1]] for i in range(p, ln))
            err = abs(want - float(score[g, k]))
            worst = max(worst, err / n_free)
            assert err <= 2e-4 * n_free, (g, k, want, score[g, k], n_free)
    print("worst beam score error per free position %.3g" % worst)


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    from sketchformer_amd import _lib
    eng, ocfg, emb, _ = _shared("small", True)
    sos, eos = _sos_eos(ocfg)
    prefix = np.ones((4, MAX_STEPS + 1), np.int64)
    kw = dict(sos=sos, eos=eos, max_steps=MAX_STEPS, prefix=prefix)
    with pytest.raises(ValueError, match="max_steps"):
        eng.greedy_decode(emb, prefix_len=[1, 1, 1, MAX_STEPS + 1], **kw)       # before any launch
    with pytest.raises(ValueError, match="out of range"):
        eng.greedy_decode(emb, prefix_len=[1, 1, 1, 1], **dict(kw, prefix=prefix * ocfg.vocab_size))
    with pytest.raises(ValueError, match="attention weights"):
        eng.greedy_decode(emb, prefix_len=[1, 1, 1, 1], with_attn_weights=True, **kw)
    lay, locfg = _build(4, blind=True)
    lay.set_flags(_lib.MODEL_DECODE_LAYERWISE)
    lemb, _ = _inputs(lay, locfg, 4, seed=8)
    for call in (lay.greedy_decode, lambda *a, **k: lay.sample_decode(*a, seed=1, **k)):
        with pytest.raises(_lib.SkfError, match="rc=-2"):                           # SKF_EUNSUPPORTED
            call(lemb, prefix_len=[1, 1, 1, 1], **kw)
    assert lay.greedy_decode(lemb, sos=sos, eos=eos, max_steps=MAX_STEPS).shape[0] == 4       # without a prefix it decodes
    cont, cocfg = _build(4, blind=True, continuous=True)
    cemb, _ = _inputs(cont, cocfg, 4, seed=8)
    with pytest.raises(ValueError, match="token models"):
        cont.greedy_decode(cemb, max_steps=MAX_STEPS, prefix=prefix, prefix_len=[1, 1, 1, 1])


# ---------------------------------------------------------------- 8. model level
def _small_model(tmp_path, batch):
    from sketchformer_amd import dataloaders, models
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=%d,num_epochs=1,log_every=4" % batch,
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "sm")
    b = model.engine.get("output/bias").copy()
    b[dataset.tokenizer.EOS] += 2.0                                # rows end at different positions
    model.engine.set("output/bias", b)
    return model, dataset


def test_complete_is_independent_of_the_chunking(tmp_path):
    from sketchformer_amd.experiments.sketch_completion import cut_sketches
    batch = 4
    model, dataset = _small_model(tmp_path, batch)
    tok = dataset.tokenizer
    x, _ = dataset.get_n_samples_from("valid", 2 * batch + 1)
    x = np.asarray(x)
    part, kept, _ = cut_sketches(x, 0.5, tok.SOS, tok.EOS)
    many = model.complete(part)
    few = model.complete(part[:3])
    L = dataset.hps["max_seq_len"]
    assert many["recon"].shape == (2 * batch + 1, L + 1) and many["recon"].dtype == np.int32
    assert np.array_equal(many["prefix_len"], kept) and np.array_equal(few["prefix_len"], kept[:3])
    assert np.array_equal(many["recon"][:3], few["recon"])
    for i in range(len(x)):
        assert many["recon"][i, 0] == tok.SOS and np.array_equal(many["recon"][i, 1:1 + kept[i]], x[i, 1:1 + kept[i]])
    a = model.complete(part[:3], mode="sample", n_samples=2, temperature=1.2, seed=1)["recon"]
    b = model.complete(part[:3], mode="sample", n_samples=2, temperature=1.2, seed=2)["recon"]
    assert a.shape == (3, 2, L + 1) and not np.array_equal(a, b)
    for i in range(3):
        assert (a[i, :, 1:1 + kept[i]] == x[i, 1:1 + kept[i]]).all()
    beams = model.complete(part[:3], mode="beam", beam_width=2)
    assert beams["recon"].shape == (3, 2, L + 1) and beams["score"].shape == (3, 2) and beams["length"].shape == (3, 2)
    assert (np.diff(beams["score"], axis=1) <= 0).all()


def test_experiment_end_to_end(tmp_path):
    from sketchformer_amd import experiments
    model, dataset = _small_model(tmp_path, 8)
    Exp = experiments.get_experiment_by_name("sketch-completion")
    for source in ("partial", "full"):
        exp = Exp(Exp.parse_hparams("n_sketches=8,source=%s,target_file=completion_%s.npz" % (source, source)), "c0", str(tmp_path))
        out = np.load(exp.compute(model), allow_pickle=True)
        L = dataset.hps["max_seq_len"]
        for key, shape in (("inputs", (8, L)), ("labels", (8,)), ("partial", (3, 8, L)), ("kept", (3, 8)), ("completion", (3, 8, L + 1)),
                           ("token_error", (3, 8)), ("dtw_distance", (3, 8)), ("class_partial", (3, 8)), ("class_completed", (3, 8)),
                           ("fraction", (3,)), ("token_error_rate", (3,)), ("dtw", (3,)), ("class_accuracy_partial", (3,)),
                           ("class_accuracy_completed", (3,))):
            assert out[key].shape == shape, (key, out[key].shape)
        assert out["fraction"].tolist() == [0.25, 0.5, 0.75] and str(out["source"]) == source
        assert ((out["token_error"] >= 0) & (out["token_error"] <= 1)).all() and np.isfinite(out["dtw_distance"]).all()
        x = out["inputs"]
        for f in range(3):
            for i in range(8):
                k = int(out["kept"][f, i])
                assert np.array_equal(out["completion"][f, i, 1:1 + k], x[i, 1:1 + k])          # the completion starts with the cut part
