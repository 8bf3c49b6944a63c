"""Sampled reconstruction on the device: temperature, top-k and nucleus decoding (include/skf.h: the selection rule).

The stand-alone launch and both decode paths are held to the rule of tests/sampling_reference.py in float64: a token is
accepted when it survives the cuts and the uniform of its (seed, stream, step) lies in its interval of the survivor CDF, give or
take 1e-4.  Rows whose survivor set would change under a perturbation of 1e-4 (`ambiguous`) are left out, at most 5 % of a case;
the inputs are built here, so those shares were checked on the host before the seeds were fixed."""
import numpy as np
import pytest
import torch

import oracle
from oracle import sketchformer_oracle
import sampling_reference as ref
from test_gpu_decode_attention import CFG2, SMALL, SMALL16, _build, _inputs, _params

pytestmark = pytest.mark.gpu

TEMPS = (0.7, 1.0, 1.3)
AMBIGUOUS_CAP = 0.05


def _uniform(seed, stream, step):
    from sketchformer_amd import ops
    return ops.sample_uniform(seed, stream, step)


# ---------------------------------------------------------------- 1. the stand-alone kernel against the rule
def standalone_cases(V, seed=3000):
    """[(name, logits (B, V) float32, k, p)]: built on the host alone (the ambiguous shares can be checked without a device)"""
    B = 64 if V <= 1004 else 32
    rng = np.random.RandomState(seed + V)
    normal = lambda: (rng.randn(B, V) * 3.0).astype(np.float32)       # noqa: E731
    out = []
    for k, p in ((0, 1.0), (8, 1.0), (0, 0.9), (8, 0.9), (V + 3, 1.0)):
        x = normal()
        if k == 0 and p < 1.0 and V >= 1004:
            # a thousand nucleus thresholds: a ramp with gaps (spacing 0.3 +- 0.05, far above the tolerance), shuffled per row
            steps = 0.3 + rng.uniform(-0.05, 0.05, size=(B, V))
            x = -np.cumsum(steps, axis=1)
            x = np.stack([row[rng.permutation(V)] for row in x]).astype(np.float32)
        out.append(("k%d_p%g" % (k, p), x, k, p))
    if V >= 52:
        for p in (1.0, 0.9):                                              # exact ties at the k-th value, across the threshold
            x = normal()
            for row in x:
                order = np.argsort(-row)
                row[order[6:11]] = row[order[7]]                          # ranks 7 .. 11 share the 8th largest value
            out.append(("ties_k8_p%g" % p, x, 8, p))
        x = normal()                                                      # rows holding -inf (never the maximum)
        for row in x:
            drop = rng.permutation(V)[:V // 3]
            row[drop[drop != row.argmax()]] = -np.inf
        out.append(("neg_inf_k8", x, 8, 1.0))
        out.append(("neg_inf_k0", x.copy(), 0, 1.0))
    return out


@pytest.mark.parametrize("V", [1, 7, 52, 64, 65, 1004, 10004])
def test_standalone_kernel_follows_the_rule(V):
    from sketchformer_amd import ops
    seed = 77
    worst, shares = 0.0, []
    for ci, (name, x, k, p) in enumerate(standalone_cases(V)):
        B = x.shape[0]
        xd = torch.from_numpy(x).cuda()
        for ti, T in enumerate(TEMPS):
            step = 3 * ci + ti
            streams = np.arange(B) * 7 + ci
            tok = ops.sample_tokens(xd, T, k, p, seed, streams.tolist(), step).cpu().numpy()
            assert tok.shape == (B,) and tok.dtype == np.int64
            skipped = 0
            for b in range(B):
                row = x[b].astype(np.float64)
                if ref.ambiguous(row, (T, k, p)):
                    skipped += 1
                    continue
                u = _uniform(seed, int(streams[b]), step)
                assert ref.accepts(row, (T, k, p), u, tok[b]), (V, name, T, b, int(tok[b]), u, ref.sample(row, (T, k, p), u))
                keep, e = ref.survivors(row, (T, k, p))
                cdf = np.cumsum(e) / e.sum()
                lo = cdf[tok[b] - 1] if tok[b] > 0 else 0.0
                worst = max(worst, lo - u, u - cdf[tok[b]])
            shares.append(skipped / B)
            assert skipped / B <= AMBIGUOUS_CAP, (V, name, T, skipped)
    print("V=%d: worst CDF excess %.3g, largest ambiguous share %.3g" % (V, worst, max(shares)))


# ---------------------------------------------------------------- 2. distribution
def test_distribution_matches_softmax():
    from sketchformer_amd import ops
    N = 8192
    row = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.9, -2.5], dtype=np.float32)
    xd = torch.from_numpy(np.tile(row, (N, 1))).cuda()
    streams = torch.arange(N, dtype=torch.int32)
    z = row.astype(np.float64) / 0.8
    for k in (0, 3):
        tok = ops.sample_tokens(xd, 0.8, k, 1.0, 5, streams, 2).cpu().numpy()
        pr = np.exp(z - z.max())
        if k:
            pr[z < np.sort(z)[-k]] = 0.0
        pr /= pr.sum()
        freq = np.bincount(tok, minlength=8)
        assert (freq[pr == 0] == 0).all()                                 # the dropped entries are never drawn
        sigma = np.sqrt(N * pr * (1 - pr))
        assert (np.abs(freq - N * pr) <= 5 * sigma).all(), (k, freq, N * pr)


# ---------------------------------------------------------------- model-level helpers
def _sos_eos(ocfg):
    return ocfg.vocab_size - 2, ocfg.vocab_size - 1


def _model(B, blind, layerwise, **kw):
    from sketchformer_amd import _lib
    eng, ocfg = _build(B, blind=blind, **kw)
    if layerwise:
        eng.set_flags(_lib.MODEL_DECODE_LAYERWISE)
    emb, tlen = _inputs(eng, ocfg, B, seed=8)
    return eng, ocfg, emb, (None if blind else tlen)


# ---------------------------------------------------------------- 3. top_k = 1 is greedy
@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
@pytest.mark.parametrize("layerwise", [False, True], ids=["fused", "layerwise"])
def test_top_k_1_is_greedy(blind, layerwise):
    eng, ocfg, emb, el = _model(4, blind, layerwise)
    sos, eos = _sos_eos(ocfg)
    want = eng.greedy_decode(emb, expected_len=el, sos=sos, eos=eos)
    got = eng.sample_decode(emb, expected_len=el, sos=sos, eos=eos, top_k=1, seed=3)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_top_k_1_is_greedy_cfg2_dimensions():
    from sketchformer_amd import engine, synthetic
    B = 4
    eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.0, use_graph=False, seed=1, **CFG2), init_seed=2)
    x, _ = synthetic.token_batch(B, CFG2["seq_len"], CFG2["vocab_size"], CFG2["n_classes"], seed=0)
    eng.encode(x)
    V = CFG2["vocab_size"]
    want = eng.greedy_decode(None, sos=V - 2, eos=V - 1)
    eng.encode(x)
    got = eng.sample_decode(None, sos=V - 2, eos=V - 1, top_k=1, top_p=0.5, temperature=0.5, seed=9)
    assert np.array_equal(got, want)


def test_top_k_1_is_greedy_bf16_model():
    B = 4
    eng, ocfg = _build(B, blind=True, act_dtype="bf16", **SMALL16)
    emb, _ = _inputs(eng, ocfg, B, seed=7)
    sos, eos = _sos_eos(ocfg)
    want = eng.greedy_decode(emb, sos=sos, eos=eos)
    assert np.array_equal(eng.sample_decode(emb, sos=sos, eos=eos, top_k=1, seed=1), want)
    other = eng.sample_decode(emb, sos=sos, eos=eos, temperature=1.5, seed=1)       # and it does draw
    assert other.shape[1] != want.shape[1] or not np.array_equal(other, want)


def test_top_k_1_is_greedy_nonblind_bf16_model_with_stream_ids():
    """A non-blind bf16 model with expected_len and stream ids of its own: the key limits and the stream ids are the two halves
    of one decode area, and both reach the one-launch kernel through the driver the fp32 model uses."""
    B = 4
    eng, ocfg = _build(B, blind=False, act_dtype="bf16", **SMALL16)
    emb, tlen = _inputs(eng, ocfg, B, seed=7)
    sos, eos = _sos_eos(ocfg)
    ids = [11, 5, 300, 2]
    want = eng.greedy_decode(emb, expected_len=tlen, sos=sos, eos=eos)
    got = eng.sample_decode(emb, expected_len=tlen, sos=sos, eos=eos, top_k=1, seed=4, stream_ids=ids)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    again = eng.sample_decode(emb, expected_len=tlen, sos=sos, eos=eos, top_k=1, seed=4, stream_ids=ids)
    assert np.array_equal(again, got)


# ---------------------------------------------------------------- 4. model decode against the oracle, step by step
def _teacher_forced_logits(P, ocfg, emb, recon, expected_len):
    """the oracle's logits of every position on the device's own prefix: (n, T, V), T = recon length - 1"""
    T = recon.shape[1] - 1
    tar = recon[:, :T]
    nattn = expected_len if expected_len is not None else T
    dummy = sketchformer_oracle.make_dummy_input(ocfg, expected_len, nattn, emb.shape[0])
    _, combined, dec_pad = sketchformer_oracle.create_masks(dummy, tar)
    return sketchformer_oracle.decode(P, ocfg, np.asarray(emb, np.float64), tar, dec_pad, combined)


def _stop_columns(recon_full, eos, seq_len):
    """columns the stop rule leaves: up to the first position after which every row has drawn an EOS"""
    seen = np.cumsum(recon_full[:, 1:] == eos, axis=1) > 0
    done = np.nonzero(seen.all(axis=0))[0]
    return (int(done[0]) + 1 if len(done) else seq_len) + 1


@pytest.mark.parametrize("blind", [True, False], ids=["blind", "nonblind"])
@pytest.mark.parametrize("layerwise", [False, True], ids=["fused", "layerwise"])
def test_sampled_decode_follows_the_oracle_step_by_step(blind, layerwise):
    B, seed = 4, 21
    eng, ocfg, emb, el = _model(B, blind, layerwise)
    sos, eos = _sos_eos(ocfg)
    b = eng.get("output/bias").copy()
    b[0] += 3.0                                   # PAD is drawn now and then: the key it masks changes every later position
    b[eos] += 2.0                                 # and some batches stop early
    eng.set("output/bias", b)
    P = _params(eng)
    streams = [11, 5, 40, 2]
    steps = skipped = pads = 0
    worst = 0.0
    for params in ((1.0, 0, 1.0), (0.7, 8, 1.0), (1.3, 0, 0.9)):
        T_, k, p = params
        recon = eng.sample_decode(emb, expected_len=el, sos=sos, eos=eos, temperature=T_, top_k=k, top_p=p, seed=seed,
                                  stream_ids=streams)
        assert recon.shape[0] == B and (recon[:, 0] == sos).all()
        # the output length obeys the stop rule (the stop test is cut to the device's own columns: it cannot see further)
        assert recon.shape[1] == _stop_columns(recon, eos, ocfg.seq_len)
        if recon.shape[1] - 1 < ocfg.seq_len:
            assert ((recon[:, 1:] == eos).sum(axis=1) > 0).all()
        logits = _teacher_forced_logits(P, ocfg, emb, recon, el)
        pads += int((recon[:, 1:-1] == 0).sum())
        for r in range(B):
            for i in range(recon.shape[1] - 1):
                steps += 1
                row = logits[r, i]
                if ref.ambiguous(row, params):
                    skipped += 1
                    continue
                u = _uniform(seed, streams[r], i)
                tok = int(recon[r, i + 1])
                assert ref.accepts(row, params, u, tok), (params, r, i, tok, u, ref.sample(row, params, u))
                keep, e = ref.survivors(row, params)
                cdf = np.cumsum(e) / e.sum()
                worst = max(worst, (cdf[tok - 1] if tok else 0.0) - u, u - cdf[tok])
    assert pads >= 1                              # a PAD inside the prefix: the teacher-forced pass masked it, so did the device
    assert skipped <= AMBIGUOUS_CAP * steps, (skipped, steps)
    print("steps %d, ambiguous %d, PAD tokens %d, worst CDF excess %.3g" % (steps, skipped, pads, worst))


# ---------------------------------------------------------------- 5. stop rule
@pytest.mark.parametrize("layerwise", [False, True], ids=["fused", "layerwise"])
def test_stop_rule(layerwise):
    eng, ocfg, emb, _ = _model(4, True, layerwise)
    sos, eos = _sos_eos(ocfg)
    b = eng.get("output/bias").copy()
    b[eos] += 50.0
    eng.set("output/bias", b)
    recon = eng.sample_decode(emb, sos=sos, eos=eos, temperature=1.2, seed=4)
    assert recon.shape == (4, 2) and (recon[:, 0] == sos).all() and (recon[:, 1] == eos).all()


# ---------------------------------------------------------------- 6. reproducibility (fused path)
def test_reproducibility_and_stream_ids():
    B = 4
    eng, ocfg, emb, _ = _model(B, True, False)
    sos, eos = _sos_eos(ocfg)
    kw = dict(sos=sos, eos=eos, temperature=1.1, top_k=20, top_p=0.95)
    a = eng.sample_decode(emb, seed=5, **kw)
    assert np.array_equal(a, eng.sample_decode(emb, seed=5, **kw))
    c = eng.sample_decode(emb, seed=6, **kw)
    assert c.shape != a.shape or not np.array_equal(a, c)
    # the same embedding in slot 0 and slot 3 with the same stream id: the same row up to and including its first EOS
    emb2 = emb.copy()
    emb2[3] = emb[0]
    d = eng.sample_decode(emb2, seed=5, stream_ids=[9, 1, 2, 9], **kw)
    n = min(d.shape[1], _first_eos(d[0], eos) + 1, _first_eos(d[3], eos) + 1)
    assert n >= 2 and np.array_equal(d[0, :n], d[3, :n])
    assert _first_eos(d[0], eos) == _first_eos(d[3], eos)


def _first_eos(row, eos):
    hit = np.nonzero(row[1:] == eos)[0]
    return int(hit[0]) + 1 if len(hit) else len(row)


def _small_model(tmp_path, batch):
    from sketchformer_amd import dataloaders, models
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=%d,num_epochs=1,log_every=4" % batch,
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "sm")
    return model, dataset


def test_sample_from_embedding_rows_are_engine_rows(tmp_path):
    model, dataset = _small_model(tmp_path, 4)
    eng, tok = model.engine, dataset.tokenizer
    b = eng.get("output/bias").copy()
    b[tok.EOS] += 2.0                             # rows end at different positions
    eng.set("output/bias", b)
    x, _ = dataset.get_n_samples_from("valid", 3)
    z = model.predict_class(x)["embedding"]
    kw = dict(temperature=0.9, top_k=30, top_p=0.97, seed=12)
    res = model.sample_from_embedding(z, n_samples=4, **kw)
    recon = res["recon"]
    L = dataset.hps["max_seq_len"] + 1
    assert recon.shape == (3, 4, L) and recon.dtype == np.int32 and res["class"].shape == (3, 4)
    flat = recon.reshape(12, L)
    ended = False
    for i in range(3):                            # chunk i of batch 4 = the four draws of embedding i, streams 4 i .. 4 i + 3
        rows = eng.sample_decode(np.repeat(z[i:i + 1], 4, axis=0), sos=tok.SOS, eos=tok.EOS, stream_ids=np.arange(4 * i, 4 * i + 4), **kw)
        for s in range(4):
            n = min(_first_eos(rows[s], tok.EOS) + 1, rows.shape[1])
            assert np.array_equal(flat[4 * i + s, :n], rows[s, :n])
            assert (flat[4 * i + s, n:] == 0).all()                          # zeros after the first EOS
            ended = ended or n < L
    assert ended
    # the result does not depend on how the rows fall into chunks: all 3 embeddings x 1 draw in one chunk, same streams
    one = model.sample_from_embedding(z, n_samples=1, **kw)["recon"]
    rows = eng.sample_decode(np.concatenate([z, z[:1]]), sos=tok.SOS, eos=tok.EOS, stream_ids=[0, 1, 2, 3], **kw)
    for i in range(3):
        n = min(_first_eos(rows[i], tok.EOS) + 1, rows.shape[1])
        assert np.array_equal(one[i, 0, :n], rows[i, :n]) and (one[i, 0, n:] == 0).all()
    same = model.sample(x, n_samples=4, **kw)["recon"]
    assert np.array_equal(same, recon)            # sample = encode on the device + sample_from_embedding


# ---------------------------------------------------------------- 7. greedy untouched
@pytest.mark.parametrize("layerwise", [False, True], ids=["fused", "layerwise"])
def test_greedy_decode_is_untouched_by_a_sampled_decode(layerwise):
    eng, ocfg, emb, _ = _model(4, True, layerwise)
    sos, eos = _sos_eos(ocfg)
    before = eng.greedy_decode(emb, sos=sos, eos=eos)
    want = oracle.predict_from_embedding(_params(eng), ocfg, emb, sos, eos)["recon"]
    assert np.array_equal(before, want)
    eng.sample_decode(emb, sos=sos, eos=eos, temperature=1.4, top_k=10, top_p=0.8, seed=2)
    assert np.array_equal(eng.greedy_decode(emb, sos=sos, eos=eos), before)


# ---------------------------------------------------------------- 8. the experiment end to end
def test_experiment_end_to_end(tmp_path):
    import os
    from sketchformer_amd import experiments
    model, dataset = _small_model(tmp_path, 8)
    Exp = experiments.get_experiment_by_name("sampled-reconstructions")
    exp = Exp(Exp.parse_hparams("n_sketches=5,n_samples=3,temperature=0.8,top_k=12,top_p=0.9,seed=3"), "s0", str(tmp_path))
    path = exp.compute(model)
    out = np.load(path, allow_pickle=True)
    L = dataset.hps["max_seq_len"]
    assert sorted(out.files) == sorted(["inputs", "labels", "greedy", "samples", "temperature", "top_k", "top_p", "seed", "n_samples",
                                        "plot"])
    assert out["inputs"].shape == (5, L) and out["labels"].shape == (5,)
    assert out["greedy"].shape == (5, L + 1) and out["samples"].shape == (5, 3, L + 1)
    assert (out["samples"][:, :, 0] == dataset.tokenizer.SOS).all()
    assert float(out["temperature"]) == np.float32(0.8) and int(out["top_k"]) == 12 and float(out["top_p"]) == np.float32(0.9)
    assert int(out["seed"]) == 3 and int(out["n_samples"]) == 3
    png = os.path.join(os.path.dirname(path), str(out["plot"]))           # the grid lies next to the .npz, in the experiment's folder
    assert os.path.isfile(png) and open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    x, _ = dataset.get_n_samples_from("valid", 5)
    assert np.array_equal(out["inputs"], x)
    assert np.array_equal(out["samples"], model.sample(x, n_samples=3, temperature=0.8, top_k=12, top_p=0.9, seed=3)["recon"])
