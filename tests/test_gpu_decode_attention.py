"""Attention weights of the greedy reconstruction (models/sketchformer.py:204,220,306 out['attn_weights']).

The reference returns the Decoder's dict of its LAST pass (builders/layers/transformer.py:328-344): a teacher-forced decoder
pass over recon[:, :T] (T = recon length - 1) with that iteration's masks.  The device writes each position's softmax rows
while it decodes (skf_model_greedy_decode_attn); every test here compares them with that teacher-forced pass of the oracle
in float64, on the engine's own parameters, embedding and reconstruction."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import sketchformer_oracle
from sketchformer_amd import synthetic

pytestmark = pytest.mark.gpu

SMALL = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
SMALL16 = dict(seq_len=40, d_model=128, num_heads=2, dff=256, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
CFG2 = dict(seq_len=200, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=1004, n_classes=345, lowerdim=128)


def _build(B, blind=True, continuous=False, act_dtype="f32", **kw):
    from sketchformer_amd import engine
    dims = dict(SMALL)
    dims.update(kw)
    if continuous:
        dims["vocab_size"] = None
    cfg = engine.make_config(batch=B, dropout_rate=0.0, use_graph=False, blind_decoder_mask=blind, continuous=continuous, seed=11,
                             act_dtype=act_dtype, **dims)
    eng = engine.TrainEngine(cfg, init_seed=1)
    ocfg = oracle.Config(dropout_rate=0.0, blind_decoder_mask=blind, continuous=continuous,
                         **{k: v for k, v in dims.items() if not (continuous and k == "vocab_size")})
    rng = np.random.RandomState(9)              # non-trivial biases / LayerNorm parameters
    for e in eng.entries:
        n = e["name"]
        if n.endswith(("/bias", "/beta", "b_attn")):
            eng.set(n, rng.normal(0, 0.1, engine.logical_shape(e)))
        elif n.endswith("/gamma"):
            eng.set(n, 1 + rng.normal(0, 0.1, engine.logical_shape(e)))
    return eng, ocfg


def _params(eng):
    return {k: v.astype(np.float64) for k, v in eng.state_dict_numpy().items()}


def _inputs(eng, ocfg, B, seed):
    """A synthetic batch and the embedding the engine's encoder makes of it (what predict hands to the decoder)."""
    if ocfg.continuous:
        x, _ = synthetic.continuous_batch(B, ocfg.seq_len, ocfg.n_classes, seed=seed)
        tlen = np.sum(x[..., -1] != 1, axis=-1)
    else:
        x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=seed)
        x[0, 7:] = 0
        x[1, 3:] = 0
        tlen = np.sum(x > 0, axis=-1)
    eng.encode(x)
    eng.synchronize()
    if ocfg.has_bottleneck:
        emb = eng.buffer("embedding").float().cpu().numpy()
    else:                                       # no bottleneck: the decoder attends to the encoder output itself
        emb = eng.buffer("enc_output").float().view(B, ocfg.seq_len, -1).cpu().numpy()
    return emb, tlen


def _oracle_weights(P, ocfg, emb, recon, expected_len):
    """The reference's last decoder pass (models/sketchformer.py:272-306): teacher-forced over recon[:, :T], masks of
    iteration T - 1.  Returns (weights dict, block1 masked (n,1,T,T) bool, block2 masked (n,1,1,L) bool)."""
    T = recon.shape[1] - 1
    tar = recon[:, :T].astype(np.float64) if ocfg.continuous else recon[:, :T]
    n = emb.shape[0]
    nattn = expected_len if expected_len is not None else T
    dummy = sketchformer_oracle.make_dummy_input(ocfg, expected_len, nattn, n)
    _, combined, dec_pad = sketchformer_oracle.create_masks(dummy, tar)
    padding_mask = np.zeros_like(dec_pad) if ocfg.blind_decoder_mask else dec_pad
    emb = np.asarray(emb, np.float64)
    pre = sketchformer_oracle.dense_expander_fwd(P, emb)[0] if ocfg.has_bottleneck else emb
    pos = sketchformer_oracle.positional_encoding(ocfg.max_pos, ocfg.d_model).astype(np.float64)
    y, _ = sketchformer_oracle._embed_fwd(P, "decoder/embedding", tar, ocfg, pos, 0.0, None)
    out = {}
    for i in range(ocfg.num_layers):
        y, w1, w2, _ = sketchformer_oracle.decoder_layer_fwd(P, "decoder/layer%d" % i, y, pre, combined, padding_mask, ocfg.num_heads,
                                                          0.0, {})
        out["decoder_layer%d_block1" % (i + 1)] = w1
        out["decoder_layer%d_block2" % (i + 1)] = w2
    return out, combined > 0, padding_mask > 0


def _check(got, recon, P, ocfg, emb, expected_len, tol=1e-4, samples=None):
    """Keys, shapes, values against the oracle, row sums, and exact zeros wherever the reference masks."""
    n, T = recon.shape[0], recon.shape[1] - 1
    H, L = ocfg.num_heads, ocfg.seq_len
    keys = ["decoder_layer%d_block%d" % (i + 1, k) for i in range(ocfg.num_layers) for k in (1, 2)]
    assert sorted(got) == sorted(keys)
    for k in keys:
        want = (n, H, T, T) if k.endswith("block1") else (n, H, T, L)
        assert got[k].shape == want and got[k].dtype == np.float32, (k, got[k].shape, want)
    idx = np.arange(n) if samples is None else np.asarray(samples)
    el = None if expected_len is None else np.asarray(expected_len)[idx]
    want, m1, m2 = _oracle_weights(P, ocfg, emb[idx], recon[idx], el)
    for k in keys:
        g = got[k][idx].astype(np.float64)
        w = want[k]
        assert w.shape == g.shape
        err = np.abs(g - w).max()
        assert err <= tol, (k, err)
        assert np.abs(g.sum(-1) - 1).max() <= 1e-5, k
        mask = np.broadcast_to(m1 if k.endswith("block1") else m2, g.shape)
        assert (w[mask] == 0).all()                              # the reference's masked entries underflow to exact zeros
        assert (g[mask] == 0).all(), (k, np.abs(g[mask]).max())
    assert m1[..., 0, 1:].all()                                  # look-ahead: block1 is exactly 0 above the diagonal
    return want


def _sos_eos(ocfg):
    return (0, 0) if ocfg.continuous else (ocfg.vocab_size - 2, ocfg.vocab_size - 1)


def _decode(eng, ocfg, emb, expected_len=None, n_valid=None):
    sos, eos = _sos_eos(ocfg)
    return eng.greedy_decode(emb, expected_len=expected_len, n_valid=n_valid, sos=sos, eos=eos, with_attn_weights=True)


def _check_recon(got, want, continuous):
    assert got.shape == want.shape, (got.shape, want.shape)
    if continuous:
        assert np.abs(got - want).max() < 2e-4 * max(1.0, np.abs(want).max())
    else:
        assert np.array_equal(got, want)


def _raise_eos_until_early_stop(eng, ocfg, P, emb, eos):
    """Raise the EOS logit until this batch stops before the last position but not at once (the slicing to T is exercised)."""
    for amount in (3.0, 2.0, 4.0, 1.5, 5.0):
        b0 = eng.get("output/bias")
        b = b0.copy(); b[eos] += amount
        eng.set("output/bias", b)
        P2 = _params(eng)
        want = oracle.predict_from_embedding(P2, ocfg, emb, ocfg.vocab_size - 2, eos)["recon"]
        if 3 < want.shape[1] < ocfg.seq_len:
            return P2, want
        eng.set("output/bias", b0)
    raise AssertionError("no EOS bias makes this batch stop early")


CASES = {"blind_early_stop": dict(), "nonblind_expected_len": dict(blind=False), "continuous": dict(continuous=True),
         "no_bottleneck": dict(lowerdim=0, do_classification=False), "attn_version2": dict(attn_version=2)}


@pytest.mark.parametrize("case,layerwise", [(c, False) for c in CASES] + [("blind_early_stop", True), ("nonblind_expected_len", True)],
                         ids=["fused-" + c for c in CASES] + ["layerwise-blind_early_stop", "layerwise-nonblind_expected_len"])
def test_decode_attention_weights_match_oracle(case, layerwise):
    """Cases 1 and 2: the one-launch-per-position kernel and the layer-by-layer path (SKF_MODEL_DECODE_LAYERWISE)."""
    from sketchformer_amd import _lib
    B = 6
    kw = dict(CASES[case])
    blind = kw.pop("blind", True)
    continuous = kw.pop("continuous", False)
    eng, ocfg = _build(B, blind=blind, continuous=continuous, **kw)
    if layerwise:
        eng.set_flags(_lib.MODEL_DECODE_LAYERWISE)
    emb, tlen = _inputs(eng, ocfg, B, seed=8)
    P = _params(eng)
    expected_len = None if blind else tlen
    n_valid = B
    if case == "blind_early_stop":
        n_valid = 4                                               # the stop test and the returned rows: first 4 samples
        P, want_recon = _raise_eos_until_early_stop(eng, ocfg, P, emb[:n_valid], ocfg.vocab_size - 1)
    else:
        want_recon = oracle.predict_from_embedding(P, ocfg, emb, *_sos_eos(ocfg), expected_len)["recon"]
    recon, weights = _decode(eng, ocfg, emb, expected_len=expected_len, n_valid=n_valid)
    _check_recon(recon, want_recon, continuous)
    assert recon.shape[0] == n_valid
    if case == "blind_early_stop":
        assert recon.shape[1] - 1 < ocfg.seq_len
    _check(weights, recon, P, ocfg, emb[:n_valid], None if expected_len is None else expected_len[:n_valid])


@pytest.mark.parametrize("blind", [True, False])
def test_decode_attention_weights_any_head_size(blind):
    """Head size 24 (outside {16, 32, 64}): layer-by-layer path through attn_decode_any_kernel."""
    B = 4
    eng, ocfg = _build(B, blind=blind, d_model=96, num_heads=4, dff=160)
    emb, tlen = _inputs(eng, ocfg, B, seed=17)
    P = _params(eng)
    expected_len = None if blind else tlen
    want_recon = oracle.predict_from_embedding(P, ocfg, emb, ocfg.vocab_size - 2, ocfg.vocab_size - 1, expected_len)["recon"]
    recon, weights = _decode(eng, ocfg, emb, expected_len=expected_len)
    _check_recon(recon, want_recon, False)
    _check(weights, recon, P, ocfg, emb, expected_len)


@pytest.mark.parametrize("continuous", [False, True], ids=["tokens", "stroke5"])
def test_capture_does_not_change_the_decode(continuous):
    """Case 3: with and without the weights, the reconstruction of each path is bit-equal; the two paths agree (tokens exactly,
    stroke-5 rows to the 2e-4 of the oracle tests: the layer-by-layer path runs its Dense layers through the GEMM kernels)."""
    from sketchformer_amd import _lib
    B = 6
    eng, ocfg = _build(B, continuous=continuous)
    emb, _ = _inputs(eng, ocfg, B, seed=5)
    sos, eos = _sos_eos(ocfg)
    res = {}
    for flags in (0, _lib.MODEL_DECODE_LAYERWISE):
        eng.set_flags(flags)
        plain = eng.greedy_decode(emb, sos=sos, eos=eos)
        recon, w = eng.greedy_decode(emb, sos=sos, eos=eos, with_attn_weights=True)
        again = eng.greedy_decode(emb, sos=sos, eos=eos)          # the weights-off path (captured step) after an eager call
        assert np.array_equal(plain, recon) and np.array_equal(plain, again)
        res[flags] = (recon, w)
    eng.set_flags(0)
    (r0, w0), (r1, w1) = res[0], res[_lib.MODEL_DECODE_LAYERWISE]
    _check_recon(r0, r1, continuous)
    for k in w0:
        assert np.abs(w0[k].astype(np.float64) - w1[k]).max() <= 1e-5, k


@pytest.mark.parametrize("blind", [True, False])
def test_bf16_model_decode_attention_weights(blind):
    """Case 4: a bf16-trained model decodes in fp32 on the master weights through the same fused kernel."""
    B = 5
    eng, ocfg = _build(B, blind=blind, act_dtype="bf16", **SMALL16)
    emb, tlen = _inputs(eng, ocfg, B, seed=7)
    P = _params(eng)
    expected_len = None if blind else tlen
    want_recon = oracle.predict_from_embedding(P, ocfg, emb, ocfg.vocab_size - 2, ocfg.vocab_size - 1, expected_len)["recon"]
    recon, weights = _decode(eng, ocfg, emb, expected_len=expected_len)
    _check_recon(recon, want_recon, False)
    _check(weights, recon, P, ocfg, emb, expected_len)


def test_decode_attention_weights_at_benchmarked_size():
    """Case 5: cfg-2 dimensions, B = 128, the seed-0 synthetic batch, blind; 4 samples over all T rows against the oracle."""
    from sketchformer_amd import engine
    B = 128
    cfg = engine.make_config(batch=B, dropout_rate=0.0, use_graph=False, seed=1, **CFG2)
    eng = engine.TrainEngine(cfg, init_seed=2)
    ocfg = oracle.Config(dropout_rate=0.0, **CFG2)
    x, _ = synthetic.token_batch(B, ocfg.seq_len, ocfg.vocab_size, ocfg.n_classes, seed=0)
    eng.encode(x)
    eng.synchronize()
    emb = eng.buffer("embedding").float().cpu().numpy()
    V = ocfg.vocab_size
    recon, weights = eng.greedy_decode(emb, sos=V - 2, eos=V - 1, with_attn_weights=True)
    assert recon.shape[0] == B
    P = _params(eng)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        _check(weights, recon, P, ocfg, emb, None, tol=2e-4, samples=[0, 41, 86, B - 1])
    finally:
        torch.set_num_threads(nthreads)


def test_nonblind_without_expected_len_is_refused(tmp_path):
    """Case 6: nattn = i + 1 changes every iteration, so the cached rows are not the reference's last pass: refused at the
    plugin, the engine and the C entry; without the flag the call behaves as before."""
    from sketchformer_amd import models, dataloaders
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=8", specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,"
                                      "blind_decoder_mask=False"), dataset, str(tmp_path), "a")
    x, _ = next(dataset.batch_iterator("train", 8, False))
    emb = model.encode_from_seq(x[:3])["embedding"]
    with pytest.raises(ValueError):
        model.predict_from_embedding(emb, with_attn_weights=True)
    out = model.predict_from_embedding(emb)
    assert out["attn_weights"] is None and out["recon"].shape[0] == 3
    # predict passes the expected length of a non-blind decoder: weights come back in the reference's keys
    got = model.predict(x[:3], with_attn_weights=True)
    T = got["recon"].shape[1] - 1
    assert sorted(got["attn_weights"]) == ["decoder_layer1_block1", "decoder_layer1_block2", "decoder_layer2_block1",
                                           "decoder_layer2_block2"]
    assert got["attn_weights"]["decoder_layer2_block2"].shape == (3, 4, T, 24)
    assert model.predict(x[:3])["attn_weights"] is None
    eng = model.engine
    with pytest.raises(ValueError):
        eng.greedy_decode(None, with_attn_weights=True)
    cfg = eng.cfg
    out = torch.zeros(cfg.batch, cfg.seq_len + 1, dtype=torch.int64, device=eng.device)
    aw = torch.zeros(2 * cfg.num_layers, cfg.batch, cfg.num_heads, cfg.seq_len, cfg.seq_len, device=eng.device)
    n_out = C.c_int(0)
    rc = eng.lib.skf_model_greedy_decode_attn(eng.handle, None, None, cfg.batch, 1, 2, cfg.seq_len, C.c_void_p(out.data_ptr()),
                                              C.byref(n_out), C.c_void_p(aw.data_ptr()), eng._stream())
    assert rc == -1                                               # SKF_EINVAL
    assert b"expected_len" in eng.lib.skf_last_error()
