"""Kernel-level parity of the bf16 path (BASELINE cfg 5), through the C ABI, against float64 references evaluated on the
SAME bf16-rounded inputs.  What is being bounded is therefore the kernels' own error: fp32 accumulation order, the bf16
rounding of P / dS as MFMA operands inside the attention kernels, and the final rounding of the stored result to bf16
(2^-9 relative).  Tolerances are stated per test; the model-level bar of SURVEY 8(c) for this path is logits <= 2e-2 rel."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _bf(a):
    """numpy -> (bf16 device tensor, float64 numpy of the rounded values)"""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(BF).cuda()
    return t, t.float().cpu().numpy().astype(np.float64)


def _f(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _close(got, want, rtol, name="", floor=1e-30):
    got = _np(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name + ": non-finite"
    scale = max(np.abs(want).max(), floor)
    err = np.abs(got - want).max() / scale
    assert err <= rtol, "%s: rel err %.3e > %.1e (scale %.3e)" % (name, err, rtol, scale)


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import _lib
    _lib.load()
    return _lib


# ------------------------------------------------------------------ Dense
@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (300, 260, 200), (1000, 1004, 512), (796, 512, 1004), (65, 36, 24), (4096, 2048, 512),
                                   (32808, 516, 512), (16384, 1024, 128)])      # the last two take the 256 x 256 tile variant
def test_gemm_bf16_nt_epilogues(lib, M, N, K):
    rng = np.random.RandomState(M + N + K)
    Kp, Np = (K + 7) // 8 * 8, (N + 7) // 8 * 8
    a = np.zeros((M, Kp)); a[:, :K] = rng.randn(M, K)
    b = np.zeros((N, Kp)); b[:, :K] = rng.randn(N, K) / np.sqrt(K)
    bias, h, c0 = rng.randn(N), rng.randn(M, Np), rng.randn(M, Np)
    A, a64 = _bf(a); Bm, b64 = _bf(b)
    H, h64 = _bf(h)
    biasd = _f(bias)
    want = a64 @ b64.T + bias
    for act, fn in ((0, lambda v: v), (1, lambda v: np.maximum(v, 0)), (2, np.tanh)):
        Cd = torch.full((M, Np), 7.0, dtype=BF, device="cuda")
        lib.call("skf_gemm_bf16", M, N, K, _p(A), Kp, _p(Bm), Kp, _p(Cd), Np, _p(biasd), act, None, 0, 0, None, 0, _s())
        _close(Cd[:, :N], fn(want), 6e-3, "nt act=%d" % act)       # one bf16 rounding of the result = 2^-9
        assert float(Cd[:, N:].float().abs().max() if Np > N else 7.0) == 7.0          # pad columns untouched
    # dgrad form: relu mask + accumulate + fp32 copy
    Cd, c64 = _bf(c0)
    C32 = torch.zeros(M, Np, dtype=torch.float32, device="cuda")
    lib.call("skf_gemm_bf16", M, N, K, _p(A), Kp, _p(Bm), Kp, _p(Cd), Np, None, 0, _p(H), Np, 1, _p(C32), Np, _s())
    w2 = (a64 @ b64.T) * (h64[:, :N] > 0) + c64[:, :N]
    _close(Cd[:, :N], w2, 6e-3, "nt relu mask + accumulate")
    _close(C32[:, :N], w2, 1e-4, "fp32 copy")                      # before the bf16 rounding: fp32 accumulation error only


@pytest.mark.parametrize("R,P,Q", [(4096, 128, 128), (3000, 512, 1008), (796, 512, 2048), (65408, 512, 512), (100, 24, 40),
                                   (16448, 264, 1008), (32768, 2048, 512)])     # R % 64 == 0, P, Q >= 256: the 256 x 256 tile variant (as 65408)
def test_gemm_bf16_wgrad(lib, R, P, Q):
    rng = np.random.RandomState(R + P + Q)
    X, x64 = _bf(rng.randn(R, P))
    dY, dy64 = _bf(rng.randn(R, Q) * np.exp(rng.randn(1, Q)))
    l = lib.load()
    splits = l.skf_gemm_bf16_wgrad_splits(P, Q, R)
    nbytes = l.skf_gemm_bf16_wgrad_workspace_bytes(P, Q, R, splits)
    slab = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    used = C.c_int(0)
    lib.call("skf_gemm_bf16_wgrad_partial", P, Q, R, _p(X), P, _p(dY), Q, splits, 1, _p(slab), nbytes, C.byref(used), _s())
    z = used.value
    dW = slab[:z * P * Q].view(z, P, Q).sum(0)
    db = slab[z * P * Q:z * P * Q + z * Q].view(z, Q).sum(0)
    scale = np.abs(x64).T @ np.abs(dy64)
    err = np.abs(_np(dW) - x64.T @ dy64) / scale
    assert err.max() < 2e-6, err.max()                              # fp32 accumulation of exact bf16 products
    _close(db, dy64.sum(0), 1e-5, "bias grad")


# ------------------------------------------------------------------ attention
def _split(x, H):
    B, L, d = x.shape
    return x.reshape(B, L, H, d // H).transpose(0, 2, 1, 3)


def _merge(x):
    B, H, L, dh = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, L, H * dh)


@pytest.mark.parametrize("B,H,Lq,Lk,causal,with_mask", [
    (2, 8, 512, 512, False, True),     # cfg-5 encoder self-attention, padding mask
    (2, 8, 511, 511, True, True),      # cfg-5 decoder self-attention, combined mask
    (2, 8, 511, 512, False, False),    # blind cross-attention
    (3, 2, 200, 130, False, True),     # ragged tiles
    (2, 2, 70, 70, True, True),
    (1, 1, 1, 1, False, False),
])
def test_attention_bf16_fwd_bwd(lib, B, H, Lq, Lk, causal, with_mask):
    dh, d = 64, 64 * H
    rng = np.random.RandomState(B * 1000 + Lq + Lk)
    Q, q = _bf(rng.randn(B, Lq, d)); K, k = _bf(rng.randn(B, Lk, d)); V, v = _bf(rng.randn(B, Lk, d))
    dO, do = _bf(rng.randn(B, Lq, d))
    km = None
    mask = np.zeros((B, 1, Lq, Lk), np.float64)
    if with_mask:
        lens = rng.randint(1, Lk + 1, size=B); lens[0] = Lk
        km = np.arange(Lk)[None, :] >= lens[:, None]
        if B > 1:
            km[1, 5:9] = True                                      # holes inside the valid range
        mask = np.maximum(mask, km[:, None, None, :].astype(np.float64))
    if causal:
        mask = np.maximum(mask, oracle.create_look_ahead_mask(Lq)[None, None])
    want_o, _, cache = oracle.sdpa_fwd(_split(q, H), _split(k, H), _split(v, H), mask)
    kmd = torch.as_tensor(km).to(torch.uint8).cuda() if km is not None else None
    O = torch.empty(B, Lq, d, dtype=BF, device="cuda")
    Olo = torch.empty(B, Lq, d, dtype=BF, device="cuda")
    stats = torch.empty(B, H, Lq, 2, dtype=torch.float32, device="cuda")
    lib.call("skf_attention_bf16_fwd", _p(Q), d, _p(K), d, _p(V), d, _p(kmd), Lk if kmd is not None else 0, int(causal), B, H, Lq,
             Lk, dh, _p(O), d, _p(Olo), _p(stats), _s())
    _close(O, _merge(want_o), 1.2e-2, "fwd")                     # P rounded to bf16 as MFMA operand + bf16 output
    assert float(Olo.float().abs().max()) <= 2.0 ** -8 * float(O.float().abs().max())      # the rounding residual of O
    # backward with the device's own (rounded) O, like the train step
    dq, dk, dv = oracle.sdpa_bwd(_split(do, H), cache)
    ws = torch.empty(B * H * Lq, dtype=torch.float32, device="cuda")
    dQ, dK, dV = (torch.full((B, L, d), 3.0, dtype=BF, device="cuda") for L in (Lq, Lk, Lk))
    lib.call("skf_attention_bf16_bwd", _p(Q), d, _p(K), d, _p(V), d, _p(O), d, _p(Olo), _p(dO), d, _p(stats), _p(kmd),
             Lk if kmd is not None else 0, int(causal), B, H, Lq, Lk, dh, _p(dQ), d, _p(dK), d, _p(dV), d, _p(ws), ws.numel() * 4, _s())
    # (floor: with a single key dQ and dK are exactly 0 and the device returns the rounding noise of delta, ~1e-7)
    _close(dQ, _merge(dq), 2e-2, "dQ", 1e-4); _close(dK, _merge(dk), 2e-2, "dK", 1e-4); _close(dV, _merge(dv), 2e-2, "dV")
    if km is not None and not causal:
        b = int(np.argmin(lens))
        if lens[b] + 128 <= Lk:                                    # whole 128-key blocks of padding: exact zeros
            first = (lens[b] + 127) // 128 * 128
            assert float(dK[b, first:].float().abs().max()) == 0.0 and float(dV[b, first:].float().abs().max()) == 0.0


@pytest.mark.parametrize("causal,Lk", [(True, 511), (False, 512)])
def test_attention_bf16_bwd_live_query_counts_is_exact(lib, causal, Lk):
    """dO is zero behind each sample's live length (decoder rows of a padded batch): with the counts the dQ pass stores zeros
    for the dead query blocks and the dK / dV pass stops early - every output equals the call without them."""
    B, H, Lq, dh = 6, 2, 511, 64
    d = H * dh
    rng = np.random.RandomState(9 + Lk)
    Q, _ = _bf(rng.randn(B, Lq, d)); K, _ = _bf(rng.randn(B, Lk, d)); V, _ = _bf(rng.randn(B, Lk, d))
    lens = np.array([0, 511, 1, 63, 130, 257], np.int32)
    do = rng.randn(B, Lq, d) * (np.arange(Lq)[None, :, None] < lens[:, None, None])
    dO, _ = _bf(do)
    O = torch.empty(B, Lq, d, dtype=BF, device="cuda"); Olo = torch.empty_like(O)
    stats = torch.empty(B, H, Lq, 2, dtype=torch.float32, device="cuda")
    lib.call("skf_attention_bf16_fwd", _p(Q), d, _p(K), d, _p(V), d, None, 0, int(causal), B, H, Lq, Lk, dh, _p(O), d, _p(Olo), _p(stats), _s())
    ws = torch.empty(B * H * Lq, dtype=torch.float32, device="cuda")
    ll = torch.as_tensor(lens).cuda()
    res = []
    for counts in (None, ll):
        dQ, dK, dV = (torch.full((B, L, d), 3.0, dtype=BF, device="cuda") for L in (Lq, Lk, Lk))
        lib.call("skf_attention_bf16_bwd_rows", _p(Q), d, _p(K), d, _p(V), d, _p(O), d, _p(Olo), _p(dO), d, _p(stats), None, 0, int(causal),
                 B, H, Lq, Lk, dh, _p(dQ), d, _p(dK), d, _p(dV), d, _p(ws), ws.numel() * 4, _p(counts), _s())
        res.append((dQ, dK, dV))
    for a, b_ in zip(res[0], res[1]):
        assert torch.equal(a, b_)
    assert float(res[1][0][0].float().abs().max()) == 0.0          # sample 0 has no live row at all


@pytest.mark.parametrize("causal", [False, True])
def test_attention_bf16_sorted_sample_list_is_a_numbering(lib, causal):
    """skf_attention_bf16_{fwd,bwd}_ordered with the list of skf_sample_order (B * H = 256: the deal over XCDs and shader engines is
    taken) or any permutation: every output bit equals the plain call."""
    from sketchformer_amd import ops
    B, H, L, dh = 32, 8, 300, 64
    d = H * dh
    rng = np.random.RandomState(31 + causal)
    Q, _ = _bf(rng.randn(B, L, d)); K, _ = _bf(rng.randn(B, L, d)); V, _ = _bf(rng.randn(B, L, d))
    lens = rng.randint(1, L + 1, size=B)
    km = torch.as_tensor(np.arange(L)[None, :] >= lens[:, None]).to(torch.uint8).cuda()
    live = torch.as_tensor(lens.astype(np.int32)).cuda()
    dO, _ = _bf(rng.randn(B, L, d) * (np.arange(L)[None, :, None] < lens[:, None, None]))
    ws = torch.empty(B * H * L, dtype=torch.float32, device="cuda")
    res = []
    for od in (None, ops.sample_order(km, None), torch.as_tensor(rng.permutation(B).astype(np.int32)).cuda()):
        O = torch.empty(B, L, d, dtype=BF, device="cuda"); Olo = torch.empty_like(O)
        stats = torch.empty(B, H, L, 2, dtype=torch.float32, device="cuda")
        lib.call("skf_attention_bf16_fwd_ordered", _p(Q), d, _p(K), d, _p(V), d, _p(km), L, int(causal), B, H, L, L, dh, _p(O), d, _p(Olo),
                 _p(stats), _p(od), _s())
        dQ, dK, dV = (torch.full((B, L, d), 3.0, dtype=BF, device="cuda") for _ in range(3))
        lib.call("skf_attention_bf16_bwd_ordered", _p(Q), d, _p(K), d, _p(V), d, _p(O), d, _p(Olo), _p(dO), d, _p(stats), _p(km), L, int(causal),
                 B, H, L, L, dh, _p(dQ), d, _p(dK), d, _p(dV), d, _p(ws), ws.numel() * 4, _p(live), _p(od), _s())
        res.append((O, Olo, stats, dQ, dK, dV))
    for r in res[1:]:
        for a, b_ in zip(res[0], r):
            assert torch.equal(a, b_)


def test_attention_bf16_fully_padded_sample_is_uniform(lib):
    B, H, L, dh = 2, 2, 130, 64
    d = H * dh
    rng = np.random.RandomState(5)
    Q, q = _bf(rng.randn(B, L, d)); K, k = _bf(rng.randn(B, L, d)); V, v = _bf(rng.randn(B, L, d))
    km = np.zeros((B, L), bool); km[1, :] = True
    O = torch.empty(B, L, d, dtype=BF, device="cuda")
    stats = torch.empty(B, H, L, 2, dtype=torch.float32, device="cuda")
    kmd = torch.as_tensor(km).to(torch.uint8).cuda()
    lib.call("skf_attention_bf16_fwd", _p(Q), d, _p(K), d, _p(V), d, _p(kmd), L, 1, B, H, L, L, dh, _p(O), d, None, _p(stats), _s())
    want = np.broadcast_to(v[1].mean(0, keepdims=True), (L, d))   # every key (look-ahead ones too) weighs 1/L
    _close(O[1], want, 1.2e-2, "all-pad sample")


# ------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("d", [128, 256, 512, 1024])        # every width skf.h promises: ldrow / strow <2>, <4>, <8>, <16>
@pytest.mark.parametrize("rate", [0.0, 0.1])
def test_layernorm_bf16_fwd_bwd(lib, d, rate):
    from sketchformer_amd import ops
    rows, site = 777, 4
    rng = np.random.RandomState(d)
    X, x = _bf(rng.randn(rows, d)); Y, y = _bf(rng.randn(rows, d)); DO, do = _bf(rng.randn(rows, d))
    g, bt = 1 + 0.1 * rng.randn(d), 0.1 * rng.randn(d)
    gd, bd = _f(g), _f(bt)
    st = ops.new_step_state("cuda", iterations=5)
    ops.step_prologue(st, seed=3)
    keep = np.ones((rows, d))
    if rate > 0:
        keep = ops.dropout_keep_mask(ops.read_step_state(st)["drop_key"], site, rate, rows * d).reshape(rows, d) / (1 - rate)
    out = torch.empty(rows, d, dtype=BF, device="cuda")
    stats = torch.empty(rows, 2, dtype=torch.float32, device="cuda")
    lib.call("skf_layernorm_residual_fwd_bf16", _p(X), _p(Y), _p(gd), _p(bd), _p(out), _p(stats), rows, d, rate, site, _p(st), _s())
    z = torch.as_tensor(x + y * keep, dtype=torch.float32).to(BF).float().numpy().astype(np.float64)   # z is stored (and normalised) rounded
    # rate 0: x + y is exact in fp32, one rounding - identical; with dropout y/(1-rate) is rounded to fp32 first and the
    # double rounding may move a value by one bf16 ulp.  Everything downstream is checked on the z the device stored.
    _close(Y, z, 1e-6 if rate == 0 else 5e-3, "z")
    z = _np(Y)
    want, cache = oracle.layernorm_fwd(z, g, bt)
    _close(out, want, 6e-3, "ln fwd")
    _close(stats[:, 0], z.mean(-1), 1e-5, "mean")
    l = lib.load()
    wsb = l.skf_layernorm_bwd_bf16_workspace_bytes(rows, d)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device="cuda")
    dz = torch.empty(rows, d, dtype=BF, device="cuda"); dy = torch.empty(rows, d, dtype=BF, device="cuda")
    dgb = torch.empty(2 * d, dtype=torch.float32, device="cuda")
    lib.call("skf_layernorm_residual_bwd_bf16", _p(DO), _p(Y), _p(stats), _p(gd), _p(dz), _p(dy), _p(dgb), C.c_void_p(dgb.data_ptr() + 4 * d),
             rows, d, rate, site, _p(st), _p(ws), wsb, _s())
    dx, dg, db = oracle.layernorm_bwd(do, cache)
    _close(dz, dx, 6e-3, "dz"); _close(dy, dx * keep, 6e-3, "dy")
    _close(dgb[:d], dg, 1e-4, "dgamma"); _close(dgb[d:], db, 1e-5, "dbeta")


@pytest.mark.parametrize("V,ld", [(1004, 1008), (52, 56)])
def test_softmax_ce_bf16(lib, V, ld):
    B, Lc = 7, 33
    rows = B * Lc
    rng = np.random.RandomState(V)
    lg = np.zeros((rows, ld)); lg[:, :V] = rng.randn(rows, V) * 3
    LG, l64 = _bf(lg)
    tgt = rng.randint(0, V, size=(B, Lc + 1)); tgt[:, 20:] = 0
    T = torch.as_tensor(tgt).cuda()
    loss = torch.empty(rows, dtype=torch.float32, device="cuda"); hit = torch.empty_like(loss)
    scale = 1.0 / rows
    lib.call("skf_softmax_ce_bf16", _p(LG), ld, rows, V, _p(T), Lc + 1, Lc, 1, 1, scale, _p(loss), _p(hit), 1, _s())
    real = tgt[:, 1:].reshape(-1)
    z = l64[:, :V]
    lse = np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1)) + z.max(-1)
    want_loss = (lse - z[np.arange(rows), real]) * (real != 0)
    _close(loss, want_loss, 1e-5, "row loss")
    assert np.array_equal(_np(hit), (z.argmax(-1) == real).astype(np.float64))
    sm = np.exp(z - lse[:, None]); sm[np.arange(rows), real] -= 1
    want_g = sm * (real != 0)[:, None] * scale
    _close(LG[:, :V], want_g, 5e-3, "in-place gradient")
    assert float(LG[:, V:].float().abs().max()) == 0.0


@pytest.mark.parametrize("L,d,U", [(40, 128, 64), (70, 512, 512), (37, 256, 128)])     # (the last two: the 1024-thread pooling / expander backward)
def test_embed_pool_expander_bf16(lib, L, d, U):
    from sketchformer_amd import engine, ops
    B, V, rate, site = 4, 52, 0.1, 2
    rng = np.random.RandomState(1)
    tok = rng.randint(0, V, size=(B, L + 1)); tok[:, 25:] = 0
    table, pos = rng.uniform(-0.05, 0.05, (V, d)), engine.positional_encoding(L + 24, d)
    st = ops.new_step_state("cuda", iterations=9)
    ops.step_prologue(st, seed=1)
    keep = ops.dropout_keep_mask(ops.read_step_state(st)["drop_key"], site, rate, B * L * d).reshape(B, L, d) / (1 - rate)
    out = torch.empty(B, L, d, dtype=BF, device="cuda")
    T = torch.as_tensor(tok).cuda()
    tabd, posd = _f(table), _f(pos)          # (kept alive: a temporary would be freed before the kernel runs)
    lib.call("skf_embed_fwd_bf16", _p(T), L + 1, B, L, _p(tabd), V, d, _p(posd), _p(out), rate, site, _p(st), _s())
    want = (table.astype(np.float32)[tok[:, :L]].astype(np.float64) * np.sqrt(d) + pos[None, :L]) * keep
    _close(out, want, 5e-3, "embed fwd")
    # pooling
    Uu, u = _bf(np.tanh(rng.randn(B, L, U))); X, x = _bf(rng.randn(B, L, d))
    Vw = rng.uniform(-0.5, 0.5, U)
    a = torch.empty(B, L, dtype=torch.float32, device="cuda"); emb = torch.empty(B, d, dtype=torch.float32, device="cuda")
    Vwd = _f(Vw)
    lib.call("skf_pool_fwd_bf16", _p(Uu), _p(Vwd), _p(X), B, L, U, d, _p(a), _p(emb), _s())
    sc = u @ Vw
    aw = np.exp(sc - sc.max(1, keepdims=True)); aw /= aw.sum(1, keepdims=True)
    _close(a, aw, 1e-5, "pool weights"); _close(emb, np.einsum("bt,btc->bc", aw, x), 1e-5, "pooled embedding")
    demb = rng.randn(B, d)
    dx = torch.empty(B, L, d, dtype=BF, device="cuda"); dV = torch.empty(U, dtype=torch.float32, device="cuda")
    ws = torch.empty(B * U, dtype=torch.float32, device="cuda")
    dembd = _f(demb)
    lib.call("skf_pool_bwd_bf16", _p(Uu), _p(Vwd), _p(X), _p(a), _p(dembd), B, L, U, d, _p(dx), _p(dV), _p(ws), ws.numel() * 4, _s())
    da = np.einsum("bc,btc->bt", demb, x)
    dsc = aw * (da - (aw * da).sum(1, keepdims=True))
    _close(dx, aw[:, :, None] * demb[:, None, :], 5e-3, "pool dx")
    _close(dV, np.einsum("bt,btu->u", dsc, u), 1e-4, "dV")
    _close(Uu, dsc[:, :, None] * Vw[None, None, :] * (1 - u * u), 6e-3, "d(pre-tanh)")
    # expander
    e, w, bias = rng.randn(B, d), rng.randn(L), rng.randn(L)
    pre = torch.empty(B, L, d, dtype=BF, device="cuda")
    ed, wd, biasd = _f(e), _f(w), _f(bias)
    lib.call("skf_expander_fwd_bf16", _p(ed), _p(wd), _p(biasd), B, L, d, _p(pre), _s())
    _close(pre, e[:, None, :] * w[None, :, None] + bias[None, :, None], 5e-3, "expander fwd")
    DP, dp = _bf(rng.randn(B, L, d))
    de = torch.ones(B, d, dtype=torch.float32, device="cuda")
    dw = torch.empty(L, dtype=torch.float32, device="cuda"); dbias = torch.empty(L, dtype=torch.float32, device="cuda")
    ws = torch.empty(2 * B * L, dtype=torch.float32, device="cuda")
    lib.call("skf_expander_bwd_bf16", _p(DP), _p(ed), _p(wd), B, L, d, _p(de), 1, _p(dw), _p(dbias), _p(ws), ws.numel() * 4, _s())
    e32 = e.astype(np.float32).astype(np.float64); w32 = w.astype(np.float32).astype(np.float64)
    _close(de, 1 + np.einsum("btc,t->bc", dp, w32), 1e-5, "expander demb (accumulated)")
    _close(dw, np.einsum("btc,bc->t", dp, e32), 1e-5, "expander dw"); _close(dbias, dp.sum((0, 2)), 1e-5, "expander dbias")


def test_cast_weight_images_and_sorted_embedding_gradient(lib):
    from sketchformer_amd import ops
    rng = np.random.RandomState(2)
    R, Cc, lds = 130, 1004, 1010
    src = np.zeros((R, lds), np.float32); src[:, :Cc] = rng.randn(R, Cc)
    S = torch.as_tensor(src).cuda()
    dst = torch.full((R, 1008), 5.0, dtype=BF, device="cuda"); dst_t = torch.full((Cc, 136), 5.0, dtype=BF, device="cuda")
    lib.call("skf_cast_weight_bf16", _p(S), R, Cc, lds, _p(dst), 1008, _p(dst_t), 136, _s())
    want = torch.as_tensor(src[:, :Cc]).to(BF)
    assert torch.equal(dst[:, :Cc].cpu(), want) and float(dst[:, Cc:].float().abs().max()) == 0.0
    assert torch.equal(dst_t[:, :R].cpu(), want.t()) and float(dst_t[:, R:].float().abs().max()) == 0.0
    # embedding gradient from bf16 dx == the fp32 kernel on the same (rounded) values
    B, L, V, d = 6, 50, 52, 128
    tok = rng.randint(0, V, size=(B, L)); tok[:, 30:] = 0
    T = torch.as_tensor(tok).cuda()
    DX, dx64 = _bf(rng.randn(B, L, d))
    l = lib.load()
    wsb = l.skf_embed_sort_workspace_bytes(B, L, V)
    ws = torch.empty(wsb + 16, dtype=torch.uint8, device="cuda")
    g16 = torch.empty(V, d, dtype=torch.float32, device="cuda"); g32 = torch.empty_like(g16)
    for out, fn, x in ((g16, "skf_embed_bwd_sorted_bf16", DX), (g32, "skf_embed_bwd_sorted", DX.float().contiguous())):
        lib.call("skf_embed_sort", _p(T), L, B, L, V, _p(out), d, _p(ws), wsb, _s())
        lib.call(fn, _p(ws), B, L, _p(x), V, d, _p(out), 0.0, 0, None, _s())
    want = np.zeros((V, d)); np.add.at(want, tok.reshape(-1), dx64.reshape(-1, d) * np.sqrt(d))
    _close(g16, want, 1e-5, "embedding gradient"); _close(g32, want, 1e-5, "embedding gradient (fp32 kernel)")


# ------------------------------------------------------------------ live row blocks (decoder-side backward of padded batches)
def _padded_rows(rng, B, Ld):
    lens = rng.randint(1, 140, size=B); lens[0] = 0; lens[1] = Ld
    tar = np.zeros((B, Ld + 1), np.int64)
    for b in range(B):
        tar[b, :lens[b] + 1] = rng.randint(1, 1000, size=lens[b] + 1)
    tar[0, 0] = 7
    live = np.concatenate([np.arange(Ld) < n for n in lens])
    return torch.as_tensor(tar).cuda(), lens, live


@pytest.mark.parametrize("N,K,relu,acc", [(512, 512, False, False), (2048, 512, True, False), (512, 1536, False, True)])
def test_gemm_bf16_dgrad_over_live_row_blocks_is_exact(lib, N, K, relu, acc):
    """cfg-5 decoder rows (128 x 511): the tiles run over the compacted live rows only; every row equals the dense call."""
    from sketchformer_amd import ops
    rng = np.random.RandomState(N + K)
    B, Ld = 128, 511
    tar, lens, live = _padded_rows(rng, B, Ld)
    M = B * Ld
    ll = ops.target_live_len(tar, Ld)
    rows1 = ops.row_blocks(ll, Ld, 1)
    assert int(rows1[0]) == int(live.sum()) and int(rows1[1]) == M
    lv = torch.as_tensor(live[:, None].astype(np.float32)).cuda()
    dy = (torch.randn(M, K, device="cuda") * lv).to(BF)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).to(BF)
    h = torch.randn(M, N, device="cuda").to(BF) if relu else None
    c0 = (torch.randn(M, N, device="cuda") * lv).to(BF)
    outs = []
    for rows in (False, True):
        c = c0.clone() if acc else torch.full((M, N), 7.0, dtype=BF, device="cuda")
        args = [M, N, K, _p(dy), K, _p(w), K, _p(c), N, None, 0, _p(h), N if relu else 0, int(acc), None, 0]
        if rows:
            lib.call("skf_gemm_bf16_rows", *args, _p(rows1), 1, _s())
        else:
            lib.call("skf_gemm_bf16", *args, _s())
        outs.append(c)
    assert torch.equal(outs[0], outs[1])
    assert float(outs[1][~torch.as_tensor(live).cuda()].float().abs().max()) == 0.0


@pytest.mark.parametrize("P,Q", [(512, 512), (512, 2048), (2048, 512)])
def test_gemm_bf16_wgrad_over_live_row_blocks(lib, P, Q):
    from sketchformer_amd import ops
    rng = np.random.RandomState(P + Q)
    B, Ld = 128, 511
    tar, lens, live = _padded_rows(rng, B, Ld)
    R = B * Ld
    b64 = ops.row_blocks(ops.target_live_len(tar, Ld), Ld, 64)
    lv = torch.as_tensor(live[:, None].astype(np.float32)).cuda()
    x = torch.randn(R, P, device="cuda").to(BF)
    dy = (torch.randn(R, Q, device="cuda") * lv).to(BF)
    l = lib.load()
    nb = l.skf_gemm_bf16_wgrad_workspace_bytes(P, Q, R, l.skf_gemm_bf16_wgrad_splits(P, Q, R))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    res = []
    for rows in (False, True):
        dw = torch.empty(P, Q, device="cuda"); db = torch.empty(Q, device="cuda")
        if rows:
            lib.call("skf_gemm_bf16_wgrad_rows", P, Q, R, _p(x), P, _p(dy), Q, _p(dw), Q, _p(db), _p(ws), nb, _p(b64), _s())
        else:
            lib.call("skf_gemm_bf16_wgrad", P, Q, R, _p(x), P, _p(dy), Q, _p(dw), Q, _p(db), _p(ws), nb, _s())
        res.append((dw, db))
    want = x.double().T @ dy.double()
    scale = (x.double().abs().T @ dy.double().abs()).cpu().numpy()
    for dw, db in res:
        err = np.abs(_np(dw) - want.cpu().numpy()) / scale
        assert err.max() < 2e-6, err.max()                       # fp32 accumulation of exact bf16 products
        _close(db, dy.double().sum(0).cpu().numpy(), 1e-5, "bias grad")


# ------------------------------------------------------------------ LayerNorm backward with a live-row list
@pytest.mark.parametrize("rate", [pytest.param(0.0, id="no-dropout"), pytest.param(0.1, id="dropout")])
@pytest.mark.parametrize("d", [pytest.param(128, id="d128-ldrow<2>"), pytest.param(1024, id="d1024-ldrow<16>-widest-lds-tile")])
def test_layernorm_bf16_bwd_rows_with_live_len(lib, d, rate):
    """Rows behind a sample's live length carry dout == 0 exactly: with the list zeros are stored for them without reading - dz, dy and
    dgamma | dbeta equal the dense call bit for bit."""
    from sketchformer_amd import ops
    B, rps, site = 6, 37, 4
    live = np.array([0, 37, 1, 36, 5, 20], np.int32)
    rows = B * rps
    dead = (np.arange(rps)[None, :] >= live[:, None]).reshape(-1)
    rng = np.random.RandomState(d + 7)
    X, _ = _bf(rng.randn(rows, d)); Y, _ = _bf(rng.randn(rows, d))
    DO, _ = _bf(rng.randn(rows, d) * ~dead[:, None])
    gd, bd = _f(1 + 0.1 * rng.randn(d)), _f(0.1 * rng.randn(d))
    st = ops.new_step_state("cuda", iterations=5)
    ops.step_prologue(st, seed=3)
    out = torch.empty(rows, d, dtype=BF, device="cuda")
    stats = torch.empty(rows, 2, dtype=torch.float32, device="cuda")
    lib.call("skf_layernorm_residual_fwd_bf16", _p(X), _p(Y), _p(gd), _p(bd), _p(out), _p(stats), rows, d, rate, site, _p(st), _s())
    wsb = lib.load().skf_layernorm_bwd_bf16_workspace_bytes(rows, d)
    ll = torch.as_tensor(live).cuda()
    res = []
    for counts in (None, ll):
        ws = torch.full((wsb // 4,), 3.0, dtype=torch.float32, device="cuda")
        dz, dy = (torch.full((rows + 1, d), 3.0, dtype=BF, device="cuda") for _ in range(2))
        dgb = torch.full((2 * d + 2,), 3.0, dtype=torch.float32, device="cuda")
        lib.call("skf_layernorm_residual_bwd_bf16_rows", _p(DO), _p(Y), _p(stats), _p(gd), _p(dz), _p(dy), _p(dgb), C.c_void_p(dgb.data_ptr() + 4 * d),
                 rows, d, rate, site, _p(st), _p(ws), wsb, _p(counts), rps if counts is not None else 0, _s())
        res.append((dz, dy, dgb))
    for a, b_ in zip(res[0], res[1]):
        assert torch.equal(a, b_)
    dz, dy, dgb = res[1]
    dd = torch.as_tensor(dead).cuda()
    assert float(dz[:rows][dd].float().abs().max()) == 0.0 and float(dy[:rows][dd].float().abs().max()) == 0.0
    assert float(dz[:rows][~dd].float().abs().max()) > 0.0
    assert float(dz[rows].float().min()) == float(dz[rows].float().max()) == 3.0 and float(dy[rows].float().min()) == float(dy[rows].float().max()) == 3.0
    assert dgb[2 * d:].tolist() == [3.0, 3.0]


# ------------------------------------------------------------------ casts at the fp32 <-> bf16 seams
def _special_floats():
    """+-0, subnormals, +-inf, the largest finite float (rounds to inf), exact ties with an even and an odd kept bit, neighbours of a
    tie, NaNs (their payload is not compared)"""
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00018000, 0x00017fff, 0x7f800000, 0xff800000,
                     0x7f7fffff, 0xff7fffff, 0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f808001, 0x3f807fff, 0x3f818001, 0x3f817fff,
                     0x7fc00000, 0x7f800001, 0xffc12345], np.uint32)
    return bits.view(np.float32)


@pytest.mark.parametrize("n", [pytest.param(1, id="n1-odd-tail-only"), pytest.param(2, id="n2-one-pair"), pytest.param(511, id="n511-pairs-and-tail"),
                               pytest.param(512, id="n512-one-workgroup"), pytest.param(513, id="n513-second-workgroup-tail"),
                               pytest.param(524289, id="n524289-second-grid-sweep-tail")])
def test_cast_f32_to_bf16_rounds_to_nearest_even(lib, n):
    rng = np.random.RandomState(n)
    sp = _special_floats()
    if n <= 2:
        sources = [sp[k:k + n].copy() for k in range(len(sp) - n + 1)]   # every special value as the tail element / in a pair
    else:
        src = (rng.randn(n) * np.exp(4 * rng.randn(n))).astype(np.float32)
        src[:len(sp)] = sp                                             # in the pairs (v_cvt_pk_bf16_f32) ...
        src[n - len(sp):] = sp[::-1]                                   # ... and, n odd, sp[0] as the tail element (the integer rounding)
        sources = [src]
    for src in sources:
        S = torch.as_tensor(src).cuda()
        dst = torch.full((n + 3,), 5.0, dtype=BF, device="cuda")
        lib.call("skf_cast_f32_to_bf16", _p(S), _p(dst), n, _s())
        want = torch.as_tensor(src).to(BF)
        got = dst[:n].cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])   # bit for bit, the sign of zero included
        assert dst[n:].float().tolist() == [5.0] * 3
    with pytest.raises(lib.SkfError):
        lib.call("skf_cast_f32_to_bf16", _p(S), C.c_void_p(dst.data_ptr() + 2), 1, _s())  # dst at a 2-byte offset
    back = torch.full((n + 3,), 5.0, dtype=torch.float32, device="cuda")
    lib.call("skf_cast_bf16_to_f32", _p(dst), _p(back), n, _s())
    assert torch.equal(back[:n].cpu().view(torch.int32), got.float().view(torch.int32)) and back[n:].tolist() == [5.0] * 3


def test_cast_bf16_to_f32_is_exact_for_every_bit_pattern(lib):
    n = 65536 + 1                                                      # every pattern once, and an odd count
    bits = np.arange(n, dtype=np.int64).astype(np.uint16).view(np.int16)
    src = torch.as_tensor(bits).view(BF).cuda()
    dst = torch.full((n + 3,), 5.0, dtype=torch.float32, device="cuda")
    lib.call("skf_cast_bf16_to_f32", _p(src), _p(dst), n, _s())
    want = (np.arange(n, dtype=np.int64).astype(np.uint16).astype(np.uint32) << 16).view(np.int32)
    assert np.array_equal(dst[:n].cpu().view(torch.int32).numpy(), want) and dst[n:].tolist() == [5.0] * 3


def test_cast_weight_bf16_batch_equals_the_single_calls(lib):
    """Four descriptors in one launch (the descriptor search, a 1 x 1 problem, dst only, dst_t only): every image equals the one
    skf_cast_weight_bf16 writes, pad columns are zero, the row behind each image keeps its sentinel."""
    rng = np.random.RandomState(8)
    l = lib.load()
    forms = [("130x1004-both", 130, 1004, 1010, 1008, 136), ("1x1-both", 1, 1, 3, 8, 8), ("33x65-dst-only", 33, 65, 65, 72, 0),
             ("64x32-dst_t-only", 64, 32, 40, 0, 72)]
    descs = (lib.SkfCastDesc * len(forms))()
    keep, begin = [], 0
    for i, (name, R, Cc, lds, ldd, ldt) in enumerate(forms):
        src = np.zeros((R, lds), np.float32); src[:, :Cc] = rng.randn(R, Cc); src[:, Cc:] = 9.0     # (the source's own pad is never read)
        S = torch.as_tensor(src).cuda()
        imgs = []
        for _ in range(2):                                               # batch, single
            dst = torch.full((R + 1, ldd), 5.0, dtype=BF, device="cuda") if ldd else None
            dst_t = torch.full((Cc + 1, ldt), 5.0, dtype=BF, device="cuda") if ldt else None
            imgs.append((dst, dst_t))
        bx = C.c_int(0)
        blocks = l.skf_cast_weight_bf16_blocks(R, Cc, ldd, ldt, C.byref(bx))
        d = descs[i]
        d.src, d.dst, d.dst_t = S.data_ptr(), (imgs[0][0].data_ptr() if ldd else None), (imgs[0][1].data_ptr() if ldt else None)
        d.R, d.C, d.ld_src, d.ld_dst, d.ld_t, d.block_begin, d.blocks_x, d.pad = R, Cc, lds, ldd, ldt, begin, bx.value, 0
        begin += blocks
        lib.call("skf_cast_weight_bf16", _p(S), R, Cc, lds, _p(imgs[1][0]), ldd, _p(imgs[1][1]), ldt, _s())
        keep.append((name, R, Cc, src, S, imgs))
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    lib.call("skf_cast_weight_bf16_batch", _p(table), len(forms), begin, _s())
    for name, R, Cc, src, S, imgs in keep:
        want = torch.as_tensor(src[:, :Cc]).to(BF)
        for k, (a, b_) in enumerate(zip(imgs[0], imgs[1])):
            if a is None:
                continue
            assert torch.equal(a, b_), name                              # bit for bit the single call
            w = want if k == 0 else want.t()
            rr, cc = w.shape
            assert torch.equal(a[:rr, :cc].cpu(), w), name
            assert float(a[:rr, cc:].float().abs().max() if a.shape[1] > cc else 0.0) == 0.0, name       # pad columns
            assert float(a[rr].float().min()) == float(a[rr].float().max()) == 5.0, name                 # sentinel row behind the image
