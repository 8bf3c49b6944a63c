"""Train-step parity: the HIP path (C ABI, skf_model_*) against the CPU oracle on
identical parameters and inputs - forward logits, argmax, losses, every gradient,
and a short Adam trajectory; plus the analytic known-answer tests of SURVEY 8(c)
at the full BASELINE size."""
import os

import numpy as np
import pytest
import torch

import oracle
from sketchformer_amd import synthetic

pytestmark = pytest.mark.gpu


def _mk(batch, rate=0.0, use_graph=False, blind=True, **kw):
    from sketchformer_amd import engine
    small = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
    small.update(kw)
    cfg = engine.make_config(batch=batch, dropout_rate=rate, use_graph=use_graph, blind_decoder_mask=blind, seed=11, **small)
    ocfg = oracle.Config(num_layers=small["num_layers"], d_model=small["d_model"], dff=small["dff"],
                         num_heads=small["num_heads"], dropout_rate=rate, lowerdim=small["lowerdim"],
                         vocab_size=small["vocab_size"], n_classes=small["n_classes"], seq_len=small["seq_len"],
                         blind_decoder_mask=blind, attn_version=small.get("attn_version", 1),
                         class_buffer_layers=small.get("class_buffer_layers", 0),
                         class_dropout=small.get("class_dropout", 0.1), optimizer=small.get("optimizer", "adam").lower(),
                         do_classification=small.get("do_classification", True),
                         do_reconstruction=small.get("do_reconstruction", True))
    eng = engine.TrainEngine(cfg, init_seed=1)
    # make biases / LN parameters non-trivial
    rng = np.random.RandomState(9)
    for e in eng.entries:
        n = e["name"]
        if n.endswith(("/bias", "/beta", "b_attn")):
            eng.set(n, rng.normal(0, 0.1, engine.logical_shape(e)))
        elif n.endswith("/gamma"):
            eng.set(n, 1 + rng.normal(0, 0.1, engine.logical_shape(e)))
    return eng, ocfg


def _rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)


def _drops_from_engine(eng, ocfg, B):
    from sketchformer_amd import ops
    key = ops.read_step_state(eng.state)["drop_key"]
    drops = {}
    for site, (name, tag) in enumerate(oracle.dropout_sites(ocfg)):
        if tag == "cls":                       # class-buffer dropout: (B, lowerdim) at rate class_dropout
            drops[name] = ops.dropout_keep_mask(key, site, ocfg.class_dropout, B * ocfg.lowerdim).reshape(B, ocfg.lowerdim)
            continue
        L = ocfg.seq_len if tag == "enc" else ocfg.seq_len - 1
        drops[name] = ops.dropout_keep_mask(key, site, ocfg.dropout_rate, B * L * ocfg.d_model).reshape(B, L, ocfg.d_model)
    return drops


@pytest.mark.parametrize("blind", [True, False])
def test_forward_logits_and_argmax(blind):
    B = 5
    eng, ocfg = _mk(B, blind=blind)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=2)
    x[0, 9:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    out, _ = oracle.forward(P, ocfg, x, x[:, :-1], training=False)
    eng.forward(x, training=False)
    torch.cuda.synchronize()
    logits = eng.buffer("logits").cpu().numpy().reshape(B, ocfg.seq_len - 1, -1)
    assert _rel(logits, out["recon"]) < 1e-4          # north star: 1e-3 rel
    assert _rel(eng.buffer("embedding").cpu().numpy(), out["embedding"]) < 1e-4
    assert _rel(eng.buffer("class_probs").cpu().numpy(), out["class"]) < 1e-4
    # token argmax: identical wherever the oracle's top-2 margin exceeds 1e-4
    srt = np.sort(out["recon"], -1)
    safe = (srt[..., -1] - srt[..., -2]) > 1e-4
    assert safe.mean() > 0.9
    assert np.array_equal(logits.argmax(-1)[safe], out["recon"].argmax(-1)[safe])


@pytest.mark.parametrize("rate,use_graph", [(0.0, False), (0.1, False), (0.1, True)])
def test_losses_and_all_gradients(rate, use_graph):
    B = 6
    eng, ocfg = _mk(B, rate=rate, use_graph=use_graph)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=3)
    x[1, 7:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    drops = _drops_from_engine(eng, ocfg, B) if rate > 0 else None
    losses, out, G = oracle.loss_and_grads(P, ocfg, x, x, y, drops)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m[k] - losses[k]) < 1e-5 * max(1.0, abs(losses[k])), (k, m[k], losses[k])
    acc = (out["recon"].argmax(-1) == x[:, 1:]).mean()
    assert abs(m["recon_acc"] - acc) < 1e-6
    got = eng.state_dict_numpy("grads")
    # d loss / d(wk bias) is analytically 0 (softmax is invariant to a per-query shift of all keys' scores):
    # the oracle gives ~1e-17, fp32 gives ~1e-8 - compare those against the gradient scale of the model instead.
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst                 # acceptance bar; typically ~1e-5
    assert np.median(list(rel.values())) < 5e-5
    for k in G:
        if k.endswith("wk/bias"):
            assert np.abs(got[k]).max() < floor, k


def test_adam_trajectory_matches_oracle():
    B = 4
    eng, ocfg = _mk(B, rate=0.0, use_graph=True)
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    st = oracle.TrainState.create(P)
    st.iterations = 3000           # lr ~ 1e-3, so parameters really move
    eng.state[0] = 3000
    for step in range(4):
        x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=20 + step)
        res, losses, _, _ = oracle.train_step(st, ocfg, x, x, y)
        eng.train_step(x, y)
        torch.cuda.synchronize()
        m = eng.step_metrics()
        assert abs(m["total_loss"] - losses["total_loss"]) < 1e-3 * abs(losses["total_loss"]), (step, m, losses)
    assert eng.iterations == 3004
    run = eng.running_metrics()
    for k, v in res.items():
        assert abs(run[k] - v) < 1e-3 * max(1.0, abs(v)), (k, run[k], v)
    got = eng.state_dict_numpy()
    # wk biases have an analytically zero gradient; Adam's m/sqrt(v) turns their rounding noise into +-lr steps
    # (in the reference too), and they cannot influence the loss - they are excluded from the trajectory check.
    worst = max((np.abs(got[k] - st.params[k]).max(), k) for k in got if not k.endswith("wk/bias"))
    assert worst[0] < 5e-4, worst


def test_first_update_has_zero_lr_k7():
    """K7: Keras evaluates the schedule on iterations=0 -> weights unchanged, m=(1-b1)g, v=(1-b2)g^2."""
    eng, ocfg = _mk(3)
    x, y = synthetic.token_batch(3, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=1)
    before = eng.params.clone()
    eng.train_step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(before, eng.params)
    g = eng.grads
    assert torch.allclose(eng.adam_m, g * (1 - 0.9), rtol=1e-5, atol=1e-12)
    assert torch.allclose(eng.adam_v, g * g * (1 - 0.98), rtol=1e-4, atol=1e-14)


# ------------------------------------------------------------------ full BASELINE size (cfg 2): properties
@pytest.fixture(scope="module")
def full():
    from sketchformer_amd import engine
    cfg = engine.make_config(batch=128, dropout_rate=0.0, use_graph=True)
    return engine.TrainEngine(cfg, init_seed=0)


def test_full_size_k2_zero_output_layer(full):
    """K2: output W=0,b=0 -> recon_loss = ln(V) * (#non-pad targets)/(B*L'), recon_acc = fraction of targets == 0."""
    x, y = synthetic.token_batch(128, 200, 1004, 345, seed=0)
    full.set("output/kernel", np.zeros((128, 1004)))
    full.set("output/bias", np.zeros(1004))
    full.forward_backward(x, None, y)
    torch.cuda.synchronize()
    m = full.step_metrics()
    tgt = x[:, 1:]
    assert abs(m["recon_loss"] - np.log(1004.0) * (tgt != 0).mean()) < 1e-4
    assert abs(m["recon_acc"] - (tgt == 0).mean()) < 1e-6
    assert np.isfinite(full.grads.cpu().numpy()).all()


def test_full_size_k4a_causality(full):
    """K4a: with inp fixed, decoder logits at position t do not depend on tar_inp[:, t+1:]."""
    x, _ = synthetic.token_batch(128, 200, 1004, 345, seed=1)
    rng = np.random.RandomState(0)
    full.load_numpy({"output/kernel": rng.uniform(-0.07, 0.07, (128, 1004))})
    full.forward(x, tar=x, training=False)
    a = full.buffer("logits").clone().view(128, 199, 1004)
    tar2 = x.copy()
    t0 = 60
    tar2[:, t0 + 1:] = rng.randint(0, 1004, size=tar2[:, t0 + 1:].shape)
    full.forward(x, tar=tar2, training=False)
    b = full.buffer("logits").view(128, 199, 1004)
    torch.cuda.synchronize()
    assert torch.equal(a[:, :t0 + 1], b[:, :t0 + 1])
    assert not torch.equal(a[:, t0 + 1:], b[:, t0 + 1:])


def test_full_size_k5_pre_decoder_rank_one(full):
    """K5: pre_decoder[b,t,:] - pre_decoder[b,t',:] = (w[t]-w[t']) * emb[b,:] + const."""
    pre = full.buffer("pre_decoder").view(128, 200, 128).cpu().numpy().astype(np.float64)
    emb = full.buffer("embedding").cpu().numpy().astype(np.float64)
    w = full.get("expand/kernel")[0].astype(np.float64)
    bias = full.get("expand/bias").astype(np.float64)
    want = emb[:, None, :] * w[None, :, None] + bias[None, :, None]
    assert np.abs(pre - want).max() < 1e-5 * max(1.0, np.abs(want).max())


def test_full_size_training_agrees_between_dense_arithmetic_modes():
    """cfg 2 (the bench workload, dropout on): 40 Adam steps with the Dense matmuls on the fp32 MFMA and with the exact
    bf16x6 split (the default) from the same initial weights and batches.  Both are fp32-accurate evaluations of the same
    step, so the loss curves agree to ~1e-4 and the trained weights stay within a few 1e-3 of each other (fp32 rounding
    differences amplified by 40 updates); the bf16x3 fast mode is NOT part of this bound."""
    from sketchformer_amd import engine
    B, L, V, C = 128, 200, 1004, 345
    batches = [synthetic.token_batch(B, L, V, C, seed=s) for s in range(4)]
    runs = {}
    for mode in (0, 6):
        eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=False, seed=3, gemm_precision=mode),
                                 init_seed=0)
        losses = []
        for it in range(40):
            xs, ys = batches[it % 4]
            eng.train_step(torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda())
            losses.append(eng.step_metrics()["total_loss"])
        runs[mode] = (np.array(losses), {e["name"]: eng.get(e["name"]).astype(np.float64) for e in eng.entries[:40]})
        del eng
        torch.cuda.empty_cache()
    l0, l6 = runs[0][0], runs[6][0]
    assert np.all(np.isfinite(l0)) and np.all(np.isfinite(l6))
    assert l0[-1] < l0[5], "loss does not go down"          # lr = 0 on the first update, warm-up after
    assert np.abs(l6 - l0).max() / np.abs(l0).max() < 5e-4, np.abs(l6 - l0).max()
    for name, w0 in runs[0][1].items():
        w6 = runs[6][1][name]
        # parameters whose true gradient is ~0 (attention key biases: the softmax ignores them) random-walk under Adam's
        # normalisation in BOTH modes: bounded by the summed learning rate (40 warm-up steps: < 2e-4), not by their size
        bound = 2e-2 * np.abs(w0).max() if np.abs(w0).max() >= 1e-2 else 1e-3
        assert np.abs(w6 - w0).max() <= bound, (name, np.abs(w6 - w0).max(), np.abs(w0).max())


def test_full_size_forward_argmax_between_dense_arithmetic_modes():
    """north_star bar at the bench size: forward logits within 1e-3 relative and token argmax identical - here between the
    fp32-MFMA and the bf16x6 evaluation of the same weights (inference mode, cfg 2).  Argmax may only differ where the
    top-2 logit margin is below the fp32 noise of either evaluation (1e-4 of the logit scale)."""
    from sketchformer_amd import engine
    B, L, V, C = 128, 200, 1004, 345
    xs, _ = synthetic.token_batch(B, L, V, C, seed=5)
    out = {}
    for mode in (0, 6):          # same init seed = same weights
        eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=False, seed=3, gemm_precision=mode),
                                 init_seed=0)
        eng.forward(torch.from_numpy(xs).cuda(), training=False)
        eng.synchronize()
        out[mode] = eng.buffer("logits").cpu().numpy().astype(np.float64)
        del eng
        torch.cuda.empty_cache()
    l0, l6 = out[0], out[6]
    scale = np.abs(l0).max()
    assert np.abs(l6 - l0).max() / scale < 1e-4, np.abs(l6 - l0).max() / scale      # bar: 1e-3
    a0, a6 = l0.argmax(1), l6.argmax(1)
    top2 = np.sort(l0, axis=1)[:, -2:]
    margin = (top2[:, 1] - top2[:, 0]) / scale
    differ = a0 != a6
    assert np.all(margin[differ] < 1e-4), (differ.sum(), margin[differ].max() if differ.any() else 0)
    assert differ.mean() < 1e-3


def test_full_size_c1_class_head_k3():
    """K3 / cfg 1: one class -> class loss 0, class_acc 1 and zero gradient from that head."""
    from sketchformer_amd import engine
    eng = engine.TrainEngine(engine.make_config(batch=8, n_classes=1, dropout_rate=0.0, use_graph=False), init_seed=0)
    x, _ = synthetic.token_batch(8, 200, 1004, 1, seed=2)
    y = np.zeros((8, 1), np.int64)
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    m = eng.step_metrics()
    assert m["class_loss"] == 0.0 and m["class_acc"] == 1.0
    assert np.abs(eng.get("classify/kernel", "grads")).max() == 0.0


# ------------------------------------------------------------------ continuous stroke-5 mode (cfg 3 family)
@pytest.mark.parametrize("rate", [0.0, 0.1])
def test_continuous_mode_losses_and_gradients(rate):
    from sketchformer_amd import engine
    B = 5
    kw = dict(seq_len=24, d_model=64, num_heads=2, dff=128, num_layers=2, n_classes=7, lowerdim=32)      # dh = 32
    eng = engine.TrainEngine(engine.make_config(batch=B, continuous=True, vocab_size=None, dropout_rate=rate,
                                                use_graph=False, seed=3, **kw), init_seed=2)
    ocfg = oracle.Config(continuous=True, dropout_rate=rate, **kw)
    rng = np.random.RandomState(4)
    for e in eng.entries:
        if e["name"].endswith(("/bias", "/beta", "b_attn")):
            eng.set(e["name"], rng.normal(0, 0.1, engine.logical_shape(e)))
    x, y = synthetic.continuous_batch(B, ocfg.seq_len, ocfg.n_classes, seed=6)
    x[0, 9:] = [0, 0, 0, 0, 1]
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    drops = _drops_from_engine(eng, ocfg, B) if rate > 0 else None
    xd = x.astype(np.float64)
    losses, out, G = oracle.loss_and_grads(P, ocfg, xd, xd, y, drops)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m[k] - losses[k]) < 2e-5 * max(1.0, abs(losses[k])), (k, m[k], losses[k])
    got = eng.state_dict_numpy("grads")
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst
    eng.forward(x, training=False)
    torch.cuda.synchronize()
    ref, _ = oracle.forward(P, ocfg, xd, xd[:, :-1], training=False)
    assert _rel(eng.buffer("logits").cpu().numpy().reshape(B, -1, 5), ref["recon"]) < 1e-4


def test_k4b_pad_asymmetry_continuous():
    """K4b: contents of pad rows do not change encoder outputs at NON-pad positions (pad keys are masked), but the
    unmasked bottleneck softmax makes the embedding (hence every decoder logit) depend on them."""
    from sketchformer_amd import engine
    B = 4
    kw = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, n_classes=7, lowerdim=32)
    eng = engine.TrainEngine(engine.make_config(batch=B, continuous=True, vocab_size=None, dropout_rate=0.0, use_graph=False, **kw))
    x, _ = synthetic.continuous_batch(B, 24, 7, seed=9)
    x[:, 12:] = [0, 0, 0, 0, 1]
    eng.forward(x, training=False)
    enc_a = eng.buffer("enc_output").clone().view(B, 24, 64); emb_a = eng.buffer("embedding").clone()
    x2 = x.copy()
    x2[:, 12:, :2] = np.random.RandomState(0).normal(0, 0.5, size=x2[:, 12:, :2].shape)        # pad bit stays 1
    eng.forward(x2, training=False)
    enc_b = eng.buffer("enc_output").view(B, 24, 64); emb_b = eng.buffer("embedding")
    torch.cuda.synchronize()
    assert torch.equal(enc_a[:, :12], enc_b[:, :12])
    assert not torch.equal(enc_a[:, 12:], enc_b[:, 12:])
    assert not torch.equal(emb_a, emb_b)


# ------------------------------------------------------------------ greedy decode with a K/V cache
def _force_eos_bias(eng, ocfg, eos, amount):
    """Raise the EOS logit so that random-weight models terminate at different steps per sample."""
    b = eng.get("output/bias")
    b[eos] += amount
    eng.set("output/bias", b)


@pytest.mark.parametrize("blind", [True, False])
def test_greedy_decode_tokens_match_oracle(blind):
    B = 6
    eng, ocfg = _mk(B, blind=blind)
    sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
    x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=5)
    x[0, 7:] = 0
    x[1, 3:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    want = oracle.predict(P, ocfg, x, sos, eos)
    eng.encode(x)
    tlen = None if blind else np.sum(x > 0, axis=-1)
    got = eng.greedy_decode(None, expected_len=tlen, sos=sos, eos=eos)
    assert got.shape == want["recon"].shape == (B, ocfg.seq_len + 1)       # nobody emits EOS at random init: full length
    assert np.array_equal(got, want["recon"])
    # an explicit embedding gives the same answer, n_valid limits the stop test / the returned rows
    emb = eng.buffer("embedding").cpu().numpy()
    got2 = eng.greedy_decode(emb, expected_len=tlen, n_valid=3, sos=sos, eos=eos)
    assert np.array_equal(got2, want["recon"][:3])


def test_greedy_decode_stops_after_all_samples_emitted_eos():
    B = 4
    eng, ocfg = _mk(B)
    sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
    _force_eos_bias(eng, ocfg, eos, 3.0)
    x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=8)
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    want = oracle.predict(P, ocfg, x, sos, eos)["recon"]
    assert 2 < want.shape[1] < ocfg.seq_len + 1, want.shape               # the case really stops early
    eng.encode(x)
    got = eng.greedy_decode(None, sos=sos, eos=eos)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert (got == eos).any(axis=1).all()                                  # sticky flags: every sample has an EOS somewhere


def test_greedy_decode_pad_token_masks_later_steps():
    """A generated PAD (id 0) becomes a masked key for all later positions (create_masks on the running output)."""
    B = 3
    eng, ocfg = _mk(B)
    sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
    b = eng.get("output/bias"); b[0] += 2.5; eng.set("output/bias", b)     # PAD gets emitted often
    x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=3)
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    want = oracle.predict(P, ocfg, x, sos, eos)["recon"]
    assert (want[:, 1:] == 0).any()
    eng.encode(x)
    got = eng.greedy_decode(None, sos=sos, eos=eos)
    assert np.array_equal(got, want)


def test_greedy_decode_continuous_matches_oracle():
    from sketchformer_amd import engine
    B = 4
    kw = dict(seq_len=20, d_model=64, num_heads=2, dff=128, num_layers=2, n_classes=7, lowerdim=32)      # dh = 32
    eng = engine.TrainEngine(engine.make_config(batch=B, continuous=True, vocab_size=None, dropout_rate=0.0,
                                                use_graph=False, seed=3, **kw), init_seed=2)
    ocfg = oracle.Config(continuous=True, dropout_rate=0.0, **kw)
    rng = np.random.RandomState(4)
    for e in eng.entries:
        if e["name"].endswith(("/bias", "/beta", "b_attn")):
            eng.set(e["name"], rng.normal(0, 0.1, engine.logical_shape(e)))
    x, _ = synthetic.continuous_batch(B, ocfg.seq_len, ocfg.n_classes, seed=6)
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    want = oracle.predict(P, ocfg, x.astype(np.float64), 0, 0)["recon"]
    eng.encode(x)
    got = eng.greedy_decode(None)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got[:, 0], np.tile([0, 0, 1, 0, 0], (B, 1)))
    assert np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max())
    # forcing the 'end of sketch' pen state makes every sample finish in the same step -> early stop
    bias = eng.get("output/bias"); bias[4] += 30.0; eng.set("output/bias", bias)
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    want = oracle.predict(P, ocfg, x.astype(np.float64), 0, 0)["recon"]
    assert want.shape[1] == 2
    eng.encode(x)
    got = eng.greedy_decode(None)
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max())


def test_greedy_decode_one_launch_path_equals_layer_by_layer_at_full_size():
    """cfg-2 dimensions (4L/8H/d128/dff512, L=200, V=1004): the one-launch-per-position kernel (skf_decode_fused.hip) and the
    layer-by-layer path it replaces (51 launches per position, the one the oracle tests above pinned in round 1) emit the
    same tokens; random weights never emit EOS, so all 200 positions are compared."""
    from sketchformer_amd import engine
    B, L, V = 16, 200, 1004
    eng = engine.TrainEngine(engine.make_config(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=V,
                                                n_classes=345, lowerdim=128, dropout_rate=0.0, use_graph=False, seed=1), init_seed=2)
    x, _ = synthetic.token_batch(B, L, V, 345, seed=5)
    eng.encode(x)
    from sketchformer_amd import _lib
    fused = eng.greedy_decode(None, sos=V - 2, eos=V - 1)
    eng.set_flags(_lib.MODEL_DECODE_LAYERWISE)
    ref = eng.greedy_decode(None, sos=V - 2, eos=V - 1)
    eng.set_flags(0)
    assert np.array_equal(eng.greedy_decode(None, sos=V - 2, eos=V - 1), fused)
    assert fused.shape == ref.shape == (B, L + 1)
    assert np.array_equal(fused, ref)


# ------------------------------------------------------------------ non-default variants of the step
@pytest.mark.parametrize("kw", [dict(attn_version=2, lowerdim=128), dict(class_buffer_layers=2, class_dropout=0.2),
                                dict(attn_version=2, lowerdim=64, class_buffer_layers=1)], ids=["selfattn_v2", "class_buffers", "both"])
@pytest.mark.parametrize("rate", [0.0, 0.1])
def test_variants_losses_and_all_gradients(kw, rate):
    """SelfAttnV2 bottleneck (embedding width = lowerdim, also the K/V input width of the cross attention) and the
    class_buffer Dense+Dropout layers: logits, losses and every gradient against the oracle, identical dropout masks."""
    B = 5
    kw = dict(kw)
    if rate == 0.0:
        kw["class_dropout"] = 0.0                      # no-dropout case: switch the class-buffer dropout off as well
    eng, ocfg = _mk(B, rate=rate, **kw)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=13)
    x[2, 5:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    assert set(P) == {n for n, _, _ in oracle.param_specs(ocfg)}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    drops = _drops_from_engine(eng, ocfg, B) if rate > 0 else None
    losses, out, G = oracle.loss_and_grads(P, ocfg, x, x, y, drops)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m[k] - losses[k]) < 1e-5 * max(1.0, abs(losses[k])), (k, m[k], losses[k])
    got = eng.state_dict_numpy("grads")
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst
    assert np.median(list(rel.values())) < 5e-5
    # inference path: logits, embedding width, greedy reconstruction through the wider embedding
    eng.forward(x, training=False)
    torch.cuda.synchronize()
    ref, _ = oracle.forward(P, ocfg, x, x[:, :-1], training=False)
    assert _rel(eng.buffer("logits").cpu().numpy().reshape(B, ocfg.seq_len - 1, -1), ref["recon"]) < 1e-4
    assert eng.buffer("embedding").shape == (B, ocfg.lowerdim if ocfg.attn_version == 2 else ocfg.d_model)
    assert _rel(eng.buffer("class_probs").cpu().numpy(), ref["class"]) < 1e-4
    sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
    want = oracle.predict(P, ocfg, x, sos, eos)
    eng.encode(x)
    assert np.array_equal(eng.greedy_decode(None, sos=sos, eos=eos), want["recon"])
    assert np.array_equal(eng.buffer("class_probs").cpu().numpy().argmax(-1), want["class"])


@pytest.mark.parametrize("kw", [dict(d_model=96, num_heads=4, dff=160), dict(d_model=80, num_heads=2, dff=128, lowerdim=24),
                                dict(d_model=192, num_heads=8, dff=256, attn_version=2, lowerdim=40),
                                dict(d_model=640, num_heads=8, dff=128, num_layers=1)],
                         ids=["d96_dh24", "d80_dh40", "d192_dh24_v2", "d640_dh80"])
@pytest.mark.parametrize("rate,blind", [(0.0, True), (0.1, False)])
def test_any_width_and_head_size(kw, rate, blind):
    """The reference takes any d_model % num_heads == 0 (builders/layers/transformer.py:150-152).  Widths / head sizes outside the
    MFMA kernels' {64,128,256,512} / {16,32,64} run on the plain fp32 kernels of skf_generic.hip (LayerNorm, expander, attention,
    greedy-decode attention) and the generic GEMM: losses, every gradient, logits and greedy reconstruction against the oracle."""
    B = 4
    eng, ocfg = _mk(B, rate=rate, blind=blind, **kw)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=17)
    x[1, 6:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    assert set(P) == {n for n, _, _ in oracle.param_specs(ocfg)}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    drops = _drops_from_engine(eng, ocfg, B) if rate > 0 else None
    losses, out, G = oracle.loss_and_grads(P, ocfg, x, x, y, drops)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m[k] - losses[k]) < 1e-5 * max(1.0, abs(losses[k])), (k, m[k], losses[k])
    got = eng.state_dict_numpy("grads")
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G if not k.endswith("wk/bias")}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst
    assert np.median(list(rel.values())) < 5e-5
    eng.forward(x, training=False)
    torch.cuda.synchronize()
    ref, _ = oracle.forward(P, ocfg, x, x[:, :-1], training=False)
    assert _rel(eng.buffer("logits").cpu().numpy().reshape(B, ocfg.seq_len - 1, -1), ref["recon"]) < 1e-4
    sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
    want = oracle.predict(P, ocfg, x, sos, eos)
    eng.encode(x)
    tlen = None if blind else np.sum(x > 0, axis=-1)          # non-blind: the cross attention sees the expected length (sketchformer.py:201-221)
    assert np.array_equal(eng.greedy_decode(None, expected_len=tlen, sos=sos, eos=eos), want["recon"])
    # a one-step Adam update runs on the same buffers
    eng.train_step(x, y)
    assert np.isfinite(eng.step_metrics()["total_loss"])


@pytest.mark.parametrize("num_heads", [4, 2], ids=["dh16", "dh32"])
def test_sequences_above_208_positions(num_heads):
    """seq_len 225 = 15 key tiles: past the 13 tiles (208 positions) every other model test stays under, where head size 16 leaves
    attn_fwd<16,13,true> / skf_attention_bwd3 for the 32-tile forward and the one-pass backward (head size 32: the 32-tile forward,
    attn_bwd2).  B = 8: the step's own row-block lists, live lengths and sample order ride along.  A padded batch with one short
    row; losses and every gradient against the oracle under the bars of test_any_width_and_head_size."""
    B = 8
    eng, ocfg = _mk(B, rate=0.0, seq_len=225, d_model=64, num_heads=num_heads, num_layers=1)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=23, full=True)     # rows reach the 15th tile
    x[1, 6:] = 0
    x[3, 100:] = 0
    x[5, 210:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    losses, out, G = oracle.loss_and_grads(P, ocfg, x, x, y)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m[k] - losses[k]) < 1e-5 * max(1.0, abs(losses[k])), (k, m[k], losses[k])
    got = eng.state_dict_numpy("grads")
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G if not k.endswith("wk/bias")}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst
    assert np.median(list(rel.values())) < 5e-5


def test_host_batches_are_staged_before_the_step_reads_them():
    """train_step on HOST arrays that differ from step to step, with the caller's stream kept busy so that the host-to-device
    copies land late: the step must be ordered behind them (round 3: a single stream hand-over per step was first taken BEFORE
    the copies were enqueued - steps then read the previous batch; found by the two-rank test)."""
    B = 8
    eng, ocfg = _mk(B, rate=0.0)
    ref, _ = _mk(B, rate=0.0)
    eng.state[0] = 3000
    ref.state[0] = 3000
    batches = [synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=40 + s) for s in range(6)]
    a = torch.randn(4096, 4096, device="cuda")
    for x, y in batches:
        for _ in range(4):
            a = (a @ a).clamp_(-1, 1)                  # ~ms of work on the caller's stream in front of the copies
        eng.train_step(x, y)
    for x, y in batches:
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        torch.cuda.synchronize()
        ref.train_step(xd, yd)
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    assert eng.iterations == ref.iterations == 3006
    assert torch.equal(eng.params, ref.params)


def _fb_both_launch_forms(B, L, rate, x, y, with_graph=False, **over):
    """forward + backward with the row-owner launches and with SKF_MODEL_FFN_LAUNCHES -> (metrics, gradients) of both and whether
    every hidden unit took the same ReLU branch in both (the two forms sum the pre-activations in different orders: a unit within
    rounding of zero may take either branch and then shifts a column of dW1 - tests/relu_branches.py; seen at 1 unit in ~10^6)."""
    from sketchformer_amd import engine, _lib
    kw = dict(seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64)
    kw.update(over)
    sides = ("encoder", "decoder") if kw.get("do_reconstruction", True) else ("encoder",)
    res, masks = [], []
    for flags, graph in ((0, False), (_lib.MODEL_FFN_LAUNCHES, False)) + (((0, True),) if with_graph else ()):
        eng = engine.TrainEngine(engine.make_config(batch=B, dropout_rate=rate, use_graph=graph, seed=5, **kw), init_seed=2)
        eng.set_flags(flags)
        eng.forward_backward(x, None, y)
        torch.cuda.synchronize()
        res.append((eng.step_metrics(), eng.state_dict_numpy("grads")))
        masks.append([(eng.buffer("%s/layer%d/ffn_h" % (side, i)) > 0).cpu().numpy() for side in sides for i in range(kw["num_layers"])])
    same_branches = all(np.array_equal(m[0], mm) for m in zip(*masks) for mm in m[1:])
    if with_graph:
        return res[0], res[1], res[2], same_branches
    return res[0], res[1], same_branches


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_ffn_launch_flag_toggles_after_a_step(graph):
    """SKF_MODEL_FFN_LAUNCHES is a RUN-TIME switch (include/skf.h): toggling it on a model that has already stepped must rebuild the
    reduction descriptors (their LayerNorm-partial split counts differ between the two launch forms) and re-capture the step graph
    - round 4 only ever set it on fresh models, where a toggle failed with 'reduction sequence changed between steps' (eager) or was
    silently ignored (captured graph)."""
    from sketchformer_amd import engine, _lib
    B, L = 5, 33
    kw = dict(seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64)
    x, y = synthetic.token_batch(B, L, 1004, 345, seed=3)
    mk = lambda: engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=graph, seed=5, **kw), init_seed=2)   # noqa: E731
    grads = {}
    for flags in (0, _lib.MODEL_FFN_LAUNCHES):                 # fresh models: the two forms as the other tests pin them
        eng = mk()
        eng.set_flags(flags)
        eng.forward_backward(x, None, y)
        torch.cuda.synchronize()
        grads[flags] = eng.grads.clone()
    eng = mk()
    for flags in (0, _lib.MODEL_FFN_LAUNCHES, 0, _lib.MODEL_FFN_LAUNCHES):
        eng.set_flags(flags)
        eng.state[0] = 0                                       # same dropout key as the fresh models' first step
        eng.forward_backward(x, None, y)
        torch.cuda.synchronize()
        assert torch.equal(eng.grads, grads[flags]), flags      # bit-equal to the fresh model of that form: the flag took effect
    eng.set_flags(0)
    eng.train_step(x, y)                                       # and the optimizer half still runs after the toggles
    torch.cuda.synchronize()
    assert np.isfinite(eng.step_metrics()["total_loss"])


@pytest.mark.parametrize("case", ["all PAD", "SOS only", "one empty and one length-1 sample", "full length"])
def test_row_owner_launches_on_degenerate_batches(case):
    """The same comparison on batches at the edges of the padding structure (live-row lists with zero or one entry, attention rows that see one
    key or none, no padding at all): finite everywhere, losses equal, every gradient within 2e-5 of the largest gradient of the step."""
    B, L = 6, 40
    x, y = synthetic.token_batch(B, L, 1004, 345, seed=1, full=case == "full length")
    if case == "all PAD":
        x[:] = 0
    elif case == "SOS only":
        x[:] = 0
        x[:, 0] = 1002
    elif case == "one empty and one length-1 sample":
        x[2] = 0
        x[4, 1:] = 0
    (m0, g0), (m1, g1), same = _fb_both_launch_forms(B, L, 0.1, x, y)
    bar = 2e-5 if same else 5e-3          # a ReLU unit on the kink took different branches in the two forms
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert np.isfinite(m0[k]) and abs(m0[k] - m1[k]) <= 2e-6 * max(1.0, abs(m1[k])), (k, m0[k], m1[k])
    top = max(np.abs(v).max() for v in g1.values())
    for k in g1:
        assert np.isfinite(g0[k]).all(), k
        assert np.abs(g0[k].astype(np.float64) - g1[k]).max() <= bar * top, (k, np.abs(g0[k] - g1[k]).max(), top, same)


@pytest.mark.parametrize("over", [dict(blind_decoder_mask=False), dict(do_reconstruction=False), dict(do_classification=False),
                                  dict(lowerdim=0, do_classification=False), dict(attn_version=2), dict(class_buffer_layers=2), dict(num_layers=1), dict(num_layers=3),
                                  dict(continuous=True, vocab_size=None), dict(optimizer="SGD"), dict(num_heads=4), dict(num_heads=2)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_row_owner_launches_in_every_model_structure(over):
    """The structural options of the reference (models/sketchformer.py:63-129: expected-length cross mask, no decoder, no classifier, no
    bottleneck, SelfAttnV2, class buffers, layer counts, continuous input, head counts) at d = 128 / dff = 512, where the row-owner
    launches are in use: forward + backward against the same step on the per-Dense launches."""
    B, L = 5, 33
    if over.get("continuous"):
        x, y = synthetic.continuous_batch(B, L, 345, seed=3)
    else:
        x, y = synthetic.token_batch(B, L, 1004, 345, seed=3)
    # (third run: the same step captured into a hipGraph and replayed on ONE stream - what a missing cross-stream dependency of the
    #  eager two-stream schedule would differ from)
    (m0, g0), (m1, g1), (m2, g2), same = _fb_both_launch_forms(B, L, 0.1, x, y, with_graph=True, **over)
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert np.isfinite(m0[k]) and abs(m0[k] - m1[k]) <= 2e-6 * max(1.0, abs(m1[k])), (k, m0[k], m1[k])
        assert abs(m0[k] - m2[k]) <= 2e-6 * max(1.0, abs(m2[k])), (k, m0[k], m2[k])
    top = max(np.abs(v).max() for v in g1.values())
    bar = 2e-5 if same else 5e-3
    for k in g1:
        assert np.isfinite(g0[k]).all(), k
        assert np.abs(g0[k].astype(np.float64) - g1[k]).max() <= bar * top, (k, np.abs(g0[k] - g1[k]).max(), top, same)
        assert np.abs(g0[k].astype(np.float64) - g2[k]).max() <= bar * top, ("graph replay", k, np.abs(g0[k] - g2[k]).max(), top, same)


@pytest.mark.parametrize("B,L,rate", [(3, 37, 0.1), (1, 200, 0.0), (17, 50, 0.1), (5, 16, 0.0)])
def test_row_owner_launches_agree_with_the_launches_they_replace(B, L, rate):
    """d = 128, dff = 512 (the shapes the fused feed-forward / LayerNorm launches are built for) at row counts that are no multiple of a
    16-row tile or a 64-row sub-group: forward + backward with the row-owner launches (default) against the same step with
    SKF_MODEL_FFN_LAUNCHES (one launch per Dense / LayerNorm, builders/layers/transformer.py:194-224) - losses and every gradient."""
    x, y = synthetic.token_batch(B, L, 1004, 345, seed=B + L)
    (m0, g0), (m1, g1), same = _fb_both_launch_forms(B, L, rate, x, y)
    for k in ("recon_loss", "class_loss", "total_loss"):
        assert abs(m0[k] - m1[k]) <= 2e-6 * max(1.0, abs(m1[k])), (k, m0[k], m1[k])
    scale = np.median([np.abs(v).max() for v in g1.values()])
    # (the key-projection bias gradient is analytically zero - softmax is invariant to it - and pure rounding noise in both forms)
    worst = max((np.abs(g0[k].astype(np.float64) - g1[k]).max() / max(np.abs(g1[k]).max(), 1e-2 * scale), k) for k in g1 if not k.endswith("wk/bias"))
    assert worst[0] < (2e-5 if same else 5e-2), (worst, same)      # (per tensor: a kink unit shifts one column of dW1 by ~1e-2 of its largest entry)


@pytest.mark.parametrize("over", [dict(), dict(blind_decoder_mask=False), dict(do_reconstruction=False), dict(do_classification=False),
                                  dict(lowerdim=0, do_classification=False), dict(attn_version=2), dict(class_buffer_layers=2),
                                  dict(num_layers=1), dict(num_layers=3), dict(continuous=True, vocab_size=None), dict(optimizer="SGD")],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "default")
def test_two_stream_step_is_deterministic_in_every_model_structure(over):
    """The eager step's side-stream schedule (held weight-gradient groups, deferred input gradients, sorts) differs with the model
    structure: two engines from one seed, 25 train steps each at d = 128 / dff = 512, bit-equal parameters and moments."""
    from sketchformer_amd import engine
    B, L = 16, 50
    kw = dict(seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64)
    kw.update(over)
    engs = [engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=False, seed=9, **kw), init_seed=4) for _ in range(2)]
    mk = (lambda i: synthetic.continuous_batch(B, L, 345, seed=60 + i)) if over.get("continuous") else (lambda i: synthetic.token_batch(B, L, 1004, 345, seed=60 + i))
    batches = [mk(i) for i in range(5)]
    for step in range(25):
        x, y = batches[step % 5]
        for e in engs:
            e.train_step(x, y)
    torch.cuda.synchronize()
    a, b = engs
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert np.isfinite(a.params.cpu().numpy()).all()


@pytest.mark.parametrize("over", [dict(), dict(do_reconstruction=False)], ids=["default", "do_reconstruction=False"])
def test_call_kinds_interleaved_on_one_model_leave_no_state_behind(over):
    """What one call sets on the host (live-row lists, the side-stream preamble's events, the scheduler's queues, maps and event
    cursor) must not reach the next call of another kind.  Two engines from one seed: A takes train_step(b0), train_step(b1); B takes
    train_step(b0), an inference forward, encode, a 4-step greedy decode, a forward_backward whose gradients are dropped, then
    train_step(b1).  Parameters and both Adam moments bit-equal, two optimizer steps each.  2 layers: the smallest model with a held
    weight-gradient group and a deferred K|V input gradient; 64 x 33 = 2112 decoder rows: every d x d weight gradient is above the
    small-GEMM size (128 x 128 x rows > 2^25), so it takes the grouped slab launches and the batched reduction.  Without a decoder the
    event pool is never rewound inside the forward (and there is nothing to decode)."""
    from sketchformer_amd import engine
    B, L = 64, 34
    kw = dict(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64,
              dropout_rate=0.1, use_graph=False, seed=9)
    kw.update(over)
    a, b = (engine.TrainEngine(engine.make_config(**kw), init_seed=4) for _ in range(2))
    b0, b1, b2, b3 = (synthetic.token_batch(B, L, 1004, 345, seed=80 + i) for i in range(4))
    a.train_step(*b0)
    a.train_step(*b1)
    b.train_step(*b0)
    b.forward(b2[0], training=False)
    b.encode(b3[0])
    if kw.get("do_reconstruction", True):
        b.greedy_decode(max_steps=4)
    b.forward_backward(b2[0], None, b2[1])
    b.train_step(*b1)
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert a.iterations == 2 and b.iterations == 2


def test_inputs_staged_event_and_model_flags_reject_misuse():
    """skf_model_wait_inputs_staged before any call has staged inputs, and skf_model_set_flags with an unknown bit, fail loudly
    (SKF_EINVAL with a message); the three defined flag bits are accepted together."""
    from sketchformer_amd import engine, _lib
    eng = engine.TrainEngine(engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=1, vocab_size=52,
                                                n_classes=7, lowerdim=32, use_graph=False), init_seed=0)
    with pytest.raises(_lib.SkfError):
        _lib.call("skf_model_wait_inputs_staged", eng.handle, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.SkfError):
        eng.set_flags(8)
    eng.set_flags(_lib.MODEL_DECODE_LAYERWISE | _lib.MODEL_FFN_LAUNCHES | _lib.MODEL_TWO_STREAM_GRAPH)
    eng.set_flags(0)
    x, y = synthetic.token_batch(4, 24, 52, 7, seed=0)
    eng.train_step(x, y)
    _lib.call("skf_model_wait_inputs_staged", eng.handle, torch.cuda.current_stream().cuda_stream)     # now there is a staging copy to wait for
    torch.cuda.synchronize()


@pytest.mark.parametrize("use_graph", [False, True])
def test_device_inputs_may_be_refilled_in_place_right_after_the_call(use_graph):
    """train_step on DEVICE tensors returns before the step has run; the caller's next action may be to refill the same tensors with
    the next batch (a prefetching loader does exactly that).  The step must see the batch it was given: the library copies its inputs
    into the workspace first thing and the caller's stream waits for that copy only (skf_model_wait_inputs_staged) - it no longer
    clones the tensors.  Two engines from one seed: one is handed fresh tensors per step, the other ONE pair of tensors that is
    overwritten (with the next batch, then with garbage) immediately after every call; parameters bit-equal after 6 steps."""
    from sketchformer_amd import engine
    B, L = 32, 64
    kw = dict(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64,
              dropout_rate=0.1, seed=11, use_graph=use_graph)
    a, b = (engine.TrainEngine(engine.make_config(**kw), init_seed=5) for _ in range(2))
    batches = [synthetic.token_batch(B, L, 1004, 345, seed=300 + i) for i in range(6)]
    xd = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    yd = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
    big = torch.empty(1 << 26, device="cuda")
    for x, y in batches:
        a.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda().view(B, 1))
        xd.copy_(torch.as_tensor(x), non_blocking=False); yd.copy_(torch.as_tensor(y).view(B, 1))
        big.normal_()                                  # keeps the device busy so that the step below starts late
        b.train_step(xd, yd)
        xd.fill_(777); yd.fill_(3)                     # garbage lands in the caller's tensors while the step is still queued
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m)


@pytest.mark.parametrize("use_graph", [False, True])
def test_benchmarked_step_is_run_to_run_deterministic(use_graph):
    """Two engines from one seed take the same 40 batches at the benchmarked size (cfg 2, B = 128, dropout 0.1): parameters and both Adam
    moments bit-equal afterwards.  The eager step runs weight gradients, deferred input gradients and the sorts on a side stream; a missing
    cross-stream dependency shows up here as a difference (tools/soak_determinism.py is the long form: 1000 steps,
    profiles/r04_soak_determinism.txt).  Eager and graph replay are not bit-equal to EACH OTHER: the replayed step has no side stream and
    takes the single-stream launch forms."""
    from sketchformer_amd import engine
    B = 128
    engs = [engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=use_graph, seed=7), init_seed=3) for _ in range(2)]
    batches = [synthetic.token_batch(B, 200, 1004, 345, seed=100 + i) for i in range(4)]
    for step in range(40):
        x, y = batches[step % 4]
        for e in engs:
            e.train_step(x, y)
    torch.cuda.synchronize()
    a, b = engs
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)
    assert np.isfinite(a.params.cpu().numpy()).all() and a.iterations == 40


def test_sgd_momentum_trajectory_matches_oracle():
    """optimizer='sgd' (models/sketchformer.py:124-126): Keras SGD(schedule, momentum=0.9); the schedule is evaluated on
    the pre-increment step, so the very first update is a no-op here too."""
    B = 4
    eng, ocfg = _mk(B, rate=0.0, optimizer="sgd")
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=30)
    before = eng.params.clone()
    eng.train_step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(before, eng.params) and eng.iterations == 1     # lr(0) = 0: velocity = 0 - 0*g
    st = oracle.TrainState.create(P)
    st.iterations = 4000
    eng.state[0] = 4000
    eng.adam_m.zero_()
    for step in range(5):
        x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=40 + step)
        _, losses, _, _ = oracle.train_step(st, ocfg, x, x, y)
        eng.train_step(x, y)
        torch.cuda.synchronize()
        m = eng.step_metrics()
        assert abs(m["total_loss"] - losses["total_loss"]) < 1e-3 * abs(losses["total_loss"]), (step, m, losses)
    got = eng.state_dict_numpy()
    worst = max((np.abs(got[k] - st.params[k]).max() / max(np.abs(st.params[k]).max(), 1e-3), k) for k in got)
    assert worst[0] < 2e-4, worst
    vel = eng.state_dict_numpy("adam_m")
    worst = max((np.abs(vel[k] - st.m[k]).max() / max(np.abs(st.m[k]).max(), 1e-12), k) for k in vel if np.abs(st.m[k]).max() > 1e-9)
    assert worst[0] < 2e-3, worst


def test_bucketed_apply_gradients_equals_plain():
    """The data-parallel schedule (gradient buckets handed to a communication stream through events, optimizer per
    bucket) on one GPU, without a process group: same parameters / moments / step counter as the plain path."""
    B = 4
    res = []
    for bucketed in (False, True):
        eng, ocfg = _mk(B, rate=0.1)
        assert eng.grad_buckets()[0][0] > 0 and sum(c for _, c in eng.grad_buckets()) == eng.n_floats
        off0, cnt0 = eng.grad_buckets()[0]
        dec_first = min(e["offset"] for e in eng.entries if e["name"].startswith(("decoder/", "output/")))
        assert off0 == dec_first and off0 + cnt0 == eng.n_floats          # bucket 0 = decoder embedding .. output layer
        eng.state[0] = 3000
        for step in range(3):
            x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=50 + step)
            eng.forward_backward(x, None, y)
            eng.apply_gradients(bucketed=bucketed)
        torch.cuda.synchronize()
        assert eng.iterations == 3003
        res.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
    for a, b in zip(*res):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)                   # embedding-gradient atomics reorder sums


def test_small_batch_steps_are_bit_reproducible():
    """No atomics and no run-dependent summation order on the whole step as long as every token id has at most 64 positions
    in the batch (embedding gradient: sorted positions per id): two runs from the same state give identical bits."""
    B = 4
    runs = []
    for _ in range(2):
        eng, ocfg = _mk(B, rate=0.1)
        eng.state[0] = 2000
        for step in range(3):
            x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=70 + step)
            eng.forward_backward(x, None, y)
            eng.apply_gradients()
        torch.cuda.synchronize()
        runs.append((eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.grads.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ structural variants (models/sketchformer.py:76-108)
@pytest.mark.parametrize("kw", [dict(do_classification=False), dict(do_reconstruction=False),
                                dict(lowerdim=0, do_classification=False), dict(lowerdim=0, do_classification=False, blind=False),
                                dict(do_reconstruction=False, class_buffer_layers=1, attn_version=2, lowerdim=64)],
                         ids=["no_class_head", "no_decoder", "no_bottleneck", "no_bottleneck_masked", "classifier_only_v2"])
@pytest.mark.parametrize("rate", [0.0, 0.1])
def test_structural_variants_losses_gradients_and_inference(kw, rate):
    B = 5
    kw = dict(kw)
    blind = kw.pop("blind", True)
    if rate == 0.0:
        kw["class_dropout"] = 0.0
    eng, ocfg = _mk(B, rate=rate, blind=blind, **kw)
    x, y = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=17)
    x[3, 6:] = 0
    P = {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}
    assert set(P) == {n for n, _, _ in oracle.param_specs(ocfg)}
    eng.forward_backward(x, None, y)
    torch.cuda.synchronize()
    drops = _drops_from_engine(eng, ocfg, B) if rate > 0 else None
    losses, out, G = oracle.loss_and_grads(P, ocfg, x, x, y, drops)
    m = eng.step_metrics()
    for k in ("recon_loss", "class_loss", "total_loss"):
        want = losses.get(k, 0.0)                      # an absent head contributes 0 (sum(all_losses))
        assert abs(m[k] - want) < 1e-5 * max(1.0, abs(want)), (k, m[k], want)
    got = eng.state_dict_numpy("grads")
    floor = 1e-3 * np.median([np.abs(G[k]).max() for k in G])
    rel = {k: np.abs(got[k].astype(np.float64) - G[k]).max() / max(np.abs(G[k]).max(), floor) for k in G}
    worst = max((v, k) for k, v in rel.items())
    assert worst[0] < 1e-3, worst
    # one optimizer step over the (shorter) flat buffer, buckets consistent with the layout
    buckets = eng.grad_buckets()
    assert sum(c for _, c in buckets) == eng.n_floats and len(buckets) == (2 if ocfg.do_reconstruction else 1)
    eng.state[0] = 2000
    eng.apply_gradients(bucketed=True)
    torch.cuda.synchronize()
    assert eng.iterations == 2001 and torch.isfinite(eng.params).all()
    eng.load_numpy({k: v.astype(np.float32) for k, v in P.items()})
    # inference
    enc = oracle.encode_from_seq(P, ocfg, x)
    eng.encode(x)
    torch.cuda.synchronize()
    emb = eng.buffer("embedding").cpu().numpy()
    if ocfg.lowerdim == 0:
        assert emb.shape == (B * ocfg.seq_len, ocfg.d_model)
        assert _rel(emb.reshape(B, ocfg.seq_len, -1), enc["embedding"]) < 1e-4
    else:
        assert _rel(emb, enc["embedding"]) < 1e-4
    if ocfg.has_classifier:
        assert _rel(eng.buffer("class_probs").cpu().numpy(), enc["class"]) < 1e-4
    if ocfg.do_reconstruction:
        sos, eos = ocfg.vocab_size - 2, ocfg.vocab_size - 1
        want = oracle.predict(P, ocfg, x, sos, eos)["recon"]
        tlen = None if blind else np.sum(x > 0, axis=-1)
        assert np.array_equal(eng.greedy_decode(None, expected_len=tlen, sos=sos, eos=eos), want)
        if ocfg.lowerdim == 0:          # explicit (B, L, d) embedding
            assert np.array_equal(eng.greedy_decode(emb.reshape(B, ocfg.seq_len, -1), expected_len=tlen, sos=sos, eos=eos), want)
    else:
        with pytest.raises(Exception):
            eng.greedy_decode(None)


_TWO_STREAM_CAPTURE = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from sketchformer_amd import engine, synthetic, _lib
B, L = 16, 56
kw = dict(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64,
          dropout_rate=0.1, seed=7)
batches = [synthetic.token_batch(B, L, 1004, 345, seed=60 + i) for i in range(4)]
got = {}
for mode in (0, 2):
    for flag in ((0, _lib.MODEL_TWO_STREAM_GRAPH) if mode == 2 else (0,)):     # mode 2 without the opt-in flag: the eager launches
        eng = engine.TrainEngine(engine.make_config(use_graph=mode, **kw), init_seed=1)
        eng.set_flags(flag)
        for x, y in batches:
            eng.train_step(x, y)
        torch.cuda.synchronize()
        got[(mode, flag)] = (eng.params.clone(), eng.step_metrics()["total_loss"])
for key in ((2, 0), (2, _lib.MODEL_TWO_STREAM_GRAPH)):
    assert np.isfinite(got[key][1]) and got[(0, 0)][1] == got[key][1], (key, got[(0, 0)][1], got[key][1])
    assert torch.equal(got[(0, 0)][0], got[key][0]), key
got[2] = got[(2, _lib.MODEL_TWO_STREAM_GRAPH)]
print("TWO_STREAM_CAPTURE_OK", got[2][1])
"""


def test_two_stream_graph_capture_is_bit_equal_to_the_eager_step():
    """use_graph = 2 (round 5): the two-stream step captured into one hipGraph - the side stream enters the capture through an event
    recorded on the capturing stream and is joined back before the capture ends.  Same launches, same launch forms, same order per
    stream as the eager step: parameters after four Adam steps are bit-equal to the eager engine's (the single-stream capture,
    use_graph = 1, takes other launch forms and only agrees to rounding).
    In a process of its own: launching the multi-branch graph has crashed INSIDE the HIP runtime (hip::Graph::UpdateStreams, below
    hipGraphLaunch; rocgdb backtrace in profiles/r05y_two_stream_graph_crash.txt) when the process had built and destroyed the models of
    tests/test_gpu_bf16_model.py and of this file before - never in a fresh process, never with the eager step or the single-stream capture.
    Round 6 (include/skf.h at SKF_MODEL_TWO_STREAM_GRAPH): in the runtime's disassembly the loop over the exec's stream vector has no bound
    when one of its streams compares equal to the launch stream - nothing of libskf is on that path; a plain-HIP reproducer
    (tools/micro/graph_parallel_stream_alias.hip) did not trigger it.  The mode therefore needs the opt-in flag; without it use_graph = 2
    issues the eager launches (checked here)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TWO_STREAM_CAPTURE % root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TWO_STREAM_CAPTURE_OK" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-800:])
