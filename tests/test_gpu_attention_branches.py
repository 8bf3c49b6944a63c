"""Every kernel the fp32 attention dispatch (skf_attention_fwd_ordered / skf_attention_bwd_ordered) can launch, against the float64
oracle at the lengths where its tile grid, its masks and its LDS budget change, plus the properties every backward kernel must keep
(live lengths, sample order, strided operands, no write outside its rows) and the shapes the launches must refuse.

Bars (tests/test_gpu_ops.py::test_attention_backward_random_shapes_masks_and_live_lengths): forward 1e-4 of the tensor's maximum,
gradients 3e-4 of the tensor's maximum with floor 0.1 - for the split (bf16x6) and the SKF_PREC_F32 kernels alike.  Before the first
device run the oracle was evaluated in float32 and in float64 on every case of CASES (CPU): the worst float32 deviation is 1.3e-6
forward and 1.6e-6 on a gradient, far below a quarter of either bar, so no case carries a bar of its own."""
import collections
import ctypes as C
import json

import numpy as np
import pytest
import torch

import oracle
from sketchformer_amd import _lib
from test_gpu_ops import _attn_case, _close, _dev, _merge, _split

pytestmark = pytest.mark.gpu

F32 = _lib.PREC_F32
FWD_BAR, BWD_BAR, FLOOR = 1e-4, 3e-4, 0.1
LOG2E = 1.4426950408889634

Case = collections.namedtuple("Case", "fwd bwd dh prec two_pass causal mask Lq Lk B H")


def _c(fwd, bwd, dh, prec, two_pass, causal, mask, Lq, Lk, B=2, H=2):
    return Case(fwd, bwd, dh, prec, two_pass, causal, mask, Lq, Lk, B, H)


# kernel names as in skf_attention.hip / skf_attention_bwd2.hip / skf_attention_bwd3.hip / skf_generic.hip
F16S, F16SL, F16, F16L = "attn_fwd<16,13,true>", "attn_fwd<16,32,true>", "attn_fwd<16,13,false>", "attn_fwd<16,32,false>"
F32S, F32L, F64S, F64L, FANY = "attn_fwd<32,13,false>", "attn_fwd<32,32,false>", "attn_fwd<64,13,false>", "attn_fwd<64,32,false>", "attn_fwd_any"
BWD3, B2_16, B2_32 = "skf_attention_bwd3", "attn_bwd2<dh16>", "attn_bwd2<dh32>"
B16, B32, B64, BANY = "attn_bwd<16,4>", "attn_bwd<32,2>", "attn_bwd<64,1>", "attn_bwd_any"

# mask kinds: none | pad (lengths, lens[0] = Lk) | hole (pad + padded keys inside sample 0's valid range) | allpad (pad + the last
# sample fully padded: float32 reference, the uniform-weights rule is fp32 semantics)
CASES = [
    # ---- dh 16, split modes.  Forward <16,13,true> up to Lk 208, <16,32,true> above; backward skf_attention_bwd3 while both
    # lengths are <= 208, the one-pass attn_bwd<16,4> as soon as one side is longer
    _c(F16S, BWD3, 16, None, False, False, "none", 1, 15),
    _c(F16S, BWD3, 16, None, False, False, "pad", 17, 16),
    _c(F16S, BWD3, 16, None, False, True, "pad", 208, 208),
    _c(F16SL, B16, 16, None, False, False, "pad", 17, 300),          # mixed: the long key side leaves bwd3
    _c(F16S, B16, 16, None, False, False, "none", 300, 17),           # mixed: the long query side leaves bwd3
    _c(F16SL, B16, 16, None, False, False, "none", 209, 224),
    _c(F16SL, B16, 16, None, False, False, "pad", 224, 209),
    _c(F16SL, B16, 16, None, False, False, "hole", 255, 256),
    _c(F16SL, B16, 16, None, False, False, "allpad", 256, 255),
    _c(F16SL, B16, 16, None, False, True, "none", 257, 257),
    _c(F16SL, B16, 16, None, False, True, "pad", 300, 300),
    _c(F16SL, B16, 16, None, False, False, "pad", 497, 512),
    _c(F16SL, B16, 16, None, False, False, "hole", 512, 497),
    _c(F16SL, B16, 16, None, False, True, "pad", 512, 512),
    _c(F16SL, B16, 16, None, False, False, "allpad", 16, 512),
    # ---- dh 16, SKF_PREC_F32: forward <16,*,false>, backward attn_bwd<16,4> at every length; Lk 193 ... 208 = 13 key tiles = the
    # shared odd key tile of the non-causal kernel
    _c(F16, B16, 16, F32, False, False, "none", 1, 1),
    _c(F16, B16, 16, F32, False, False, "pad", 15, 17),
    _c(F16, B16, 16, F32, False, True, "pad", 16, 16),
    _c(F16, B16, 16, F32, False, False, "pad", 37, 193),              # shared tile, one live key in it
    _c(F16, B16, 16, F32, False, False, "hole", 100, 200),            # shared tile
    _c(F16, B16, 16, F32, False, False, "none", 208, 208),            # shared tile, full
    _c(F16, B16, 16, F32, False, False, "allpad", 53, 208),           # shared tile, a fully padded sample
    _c(F16, B16, 16, F32, False, True, "pad", 200, 200),              # 13 tiles, look-ahead: no sharing
    _c(F16L, B16, 16, F32, False, False, "pad", 209, 300),
    _c(F16L, B16, 16, F32, False, False, "none", 300, 209),
    _c(F16L, B16, 16, F32, False, False, "allpad", 256, 257),
    _c(F16L, B16, 16, F32, False, False, "hole", 497, 512),
    _c(F16L, B16, 16, F32, False, True, "pad", 512, 512),
    # ---- dh 16, split modes, SKF_ATTN_TWO_PASS: attn_bwd2<dh16> above 208 (512 = 32 query and 32 key tiles)
    _c(F16SL, B2_16, 16, None, True, True, "pad", 209, 209),
    _c(F16SL, B2_16, 16, None, True, False, "pad", 300, 209),
    _c(F16SL, B2_16, 16, None, True, False, "hole", 497, 300),
    _c(F16SL, B2_16, 16, None, True, False, "none", 512, 512),
    _c(F16SL, B2_16, 16, None, True, True, "pad", 512, 512),
    _c(F16SL, B2_16, 16, None, True, False, "allpad", 17, 512),
    # ---- dh 32, split modes: attn_bwd2<dh32> while both lengths are <= 256, the one-pass attn_bwd<32,2> above
    _c(F32S, B2_32, 32, None, False, False, "none", 1, 17),
    _c(F32S, B2_32, 32, None, False, False, "none", 17, 1),
    _c(F32S, B2_32, 32, None, False, False, "pad", 15, 16),
    _c(F32S, B2_32, 32, None, False, False, "hole", 37, 53),          # ragged on both sides
    _c(F32L, B2_32, 32, None, False, False, "pad", 208, 209),
    _c(F32L, B2_32, 32, None, False, False, "hole", 224, 255),
    _c(F32L, B2_32, 32, None, False, False, "none", 255, 224),
    _c(F32L, B2_32, 32, None, False, True, "pad", 256, 256),
    _c(F32L, B2_32, 32, None, False, False, "allpad", 256, 256),
    _c(F32L, B32, 32, None, False, False, "none", 257, 256),          # 256 | 257: bwd2 -> one-pass, query side
    _c(F32L, B32, 32, None, False, False, "pad", 256, 257),           # ... key side
    _c(F32L, B32, 32, None, False, True, "pad", 257, 257),
    _c(F32L, B32, 32, None, False, True, "none", 300, 300),
    # ---- dh 32, SKF_PREC_F32: attn_bwd<32,2> at every length (Lq <= 448: LDS); Lk 65 ... 80 = 5 key tiles = its shared odd tile
    _c(F32S, B32, 32, F32, False, False, "none", 1, 1),
    _c(F32S, B32, 32, F32, False, False, "pad", 16, 17),
    _c(F32S, B32, 32, F32, False, False, "pad", 37, 65),              # shared tile, one live key in it
    _c(F32S, B32, 32, F32, False, False, "none", 100, 72),            # shared tile
    _c(F32S, B32, 32, F32, False, False, "hole", 80, 80),             # shared tile, full
    _c(F32S, B32, 32, F32, False, False, "allpad", 53, 72),           # shared tile, a fully padded sample
    _c(F32S, B32, 32, F32, False, True, "pad", 72, 72),               # 5 tiles, look-ahead: no sharing
    _c(F32S, B32, 32, F32, False, False, "none", 448, 15),
    _c(F32L, B32, 32, F32, False, False, "hole", 300, 497),
    _c(F32L, B32, 32, F32, False, False, "pad", 448, 512),            # the longest the one-pass kernel holds
    _c(F32L, B32, 32, F32, False, True, "pad", 448, 448),
    _c(F32L, B32, 32, F32, False, False, "allpad", 17, 512),
    # ---- dh 64: forward <64,13> / <64,32> up to Lk 288, backward attn_bwd<64,1> up to Lq 224 (one key tile per wave: Lk <= 16 is
    # the single-tile case)
    _c(F64S, B64, 64, None, False, False, "none", 53, 1),
    _c(F64S, B64, 64, None, False, False, "pad", 100, 7),
    _c(F64S, B64, 64, None, False, False, "hole", 37, 16),
    _c(F64S, B64, 64, None, False, True, "none", 7, 7),
    _c(F64S, B64, 64, None, False, True, "pad", 16, 16),
    _c(F64S, B64, 64, None, False, False, "pad", 37, 53),             # ragged on both sides
    _c(F64L, B64, 64, None, False, False, "pad", 208, 209),
    _c(F64S, B64, 64, F32, False, False, "none", 209, 208),
    _c(F64L, B64, 64, None, False, False, "hole", 224, 288),          # both LDS limits at once
    _c(F64L, B64, 64, None, False, True, "pad", 224, 224),
    _c(F64L, B64, 64, None, False, False, "allpad", 100, 288),
    _c(F64L, B64, 64, F32, False, False, "none", 17, 273),
]
# ---- any other head size: attn_fwd_any / attn_bwd_q_any / attn_bwd_kv_any (one wave per row, keys lane, lane + 64, ...)
_ANY_MASKS = [(False, "none"), (False, "pad"), (True, "none"), (True, "pad"), (False, "hole"), (False, "allpad")]
_ANY_L = [1, 63, 64, 65, 200]
for _i, _dh in enumerate([8, 24, 40, 80, 128]):
    for _j, _L in enumerate(_ANY_L):
        _causal, _mask = _ANY_MASKS[(_i + 2 * _j) % len(_ANY_MASKS)]
        _Lk = _L if _causal else _ANY_L[(_j + 1 + _i % 4) % 5]          # (never _L itself)
        if _mask == "hole" and _Lk < 3:
            _mask = "pad"
        CASES.append(_c(FANY, BANY, _dh, None, False, _causal, _mask, _L, _Lk))
CASES.append(_c(FANY, BANY, 24, None, False, False, "hole", 1024, 1024, B=1, H=1))       # 16 keys per lane
CASES.append(_c(FANY, BANY, 8, None, False, True, "none", 1024, 1024, B=1, H=1))


def _id(c):
    return "dh%d-%s%s-%s%s-%dx%d" % (c.dh, "f32" if c.prec == F32 else "split", "-2pass" if c.two_pass else "",
                                     "causal+" if c.causal else "", c.mask, c.Lq, c.Lk)


def _dispatch(dh, prec, two_pass, Lq, Lk):
    """The table of skf_attention.hip restated: (forward kernel, backward kernel) of a shape."""
    split = (_lib.default_precision() if prec is None else prec) != F32
    if dh not in (16, 32, 64):
        return FANY, BANY
    fwd = "attn_fwd<%d,%d,%s>" % (dh, 13 if Lk <= 208 else 32, "true" if dh == 16 and split else "false")
    if dh == 16 and split and not two_pass and Lq <= 208 and Lk <= 208:
        return fwd, BWD3
    if split and ((dh == 16 and two_pass) or (dh == 32 and Lq <= 256 and Lk <= 256)):
        return fwd, "attn_bwd2<dh%d>" % dh
    return fwd, "attn_bwd<%d,%d>" % (dh, 64 // dh)


_TAGS = {F16S: "attn_fwd<dh16>", F16SL: "attn_fwd<dh16>", F16: "attn_fwd<dh16>", F16L: "attn_fwd<dh16>", F32S: "attn_fwd<dh32>",
         F32L: "attn_fwd<dh32>", F64S: "attn_fwd<dh64>", F64L: "attn_fwd<dh64>", FANY: "attn_fwd<any>", BWD3: "attn_bwd<dh16>",
         B16: "attn_bwd<dh16>", B2_16: "attn_bwd2<dh16,bf16x6>", B2_32: "attn_bwd2<dh32,bf16x6>", B32: "attn_bwd<dh32>",
         B64: "attn_bwd<dh64>", BANY: "attn_bwd<any>"}


class _Profiled:
    """The launch tags (SkfProfScope) of the calls made inside the block: which kernel family the dispatch reached."""

    def __enter__(self):
        torch.cuda.synchronize()
        _lib.load().skf_profiler_enable(1)
        self.tags = None
        return self

    def __exit__(self, *exc):
        lib = _lib.load()
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
                buf = C.create_string_buffer(1 << 16)
                _lib.check(lib.skf_profiler_report(buf, len(buf)), "skf_profiler_report")
                self.tags = [r["tag"] for r in json.loads(buf.value.decode())]
        finally:
            lib.skf_profiler_enable(0)


@pytest.fixture(scope="module")
def ops():
    from sketchformer_amd import ops
    return ops


_WORST = collections.defaultdict(dict)      # kernel name -> {quantity: worst observed error relative to its bar's scale}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """One line per kernel after the module ran: the figures of profiles/attention_branch_errors.txt."""
    yield
    for name in sorted(_WORST):
        print("attention-branch-error %-24s %s" % (name, "  ".join("%s %.2e" % kv for kv in sorted(_WORST[name].items()))))


def _rel_err(got, want, floor=1e-30):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "non-finite output"
    return np.abs(got - want).max() / max(np.abs(want).max(), floor)


def _hold(kernel, what, got, want, bar, floor=1e-30):
    err = _rel_err(got, want, floor)
    _WORST[kernel][what] = max(_WORST[kernel].get(what, 0.0), err)
    _close(got, want, rtol=bar, name="%s %s" % (kernel, what), floor=floor)


def _inputs(c, seed=None):
    """(q, k, v, dO) float64, key mask (bool or None), additive-mask indicator (B,1,Lq,Lk) float32."""
    seed = 7000 + 13 * c.Lq + 3 * c.Lk + c.dh if seed is None else seed
    q, k, v, do, km, mask = _attn_case(c.B, c.H, c.Lq, c.Lk, c.dh, c.causal, c.mask != "none", seed, all_pad_row=c.mask == "allpad")
    if c.mask == "hole":
        assert c.Lk >= 3
        a = min(14, c.Lk // 2)
        km[0, a:a + min(5, c.Lk - a - 1)] = True             # across the first tile boundary when the keys reach that far
        mask = km[:, None, None, :].astype(np.float32) * np.ones((1, 1, c.Lq, 1), np.float32)
        if c.causal:
            mask = np.maximum(mask, oracle.create_look_ahead_mask(c.Lq)[None, None])
    return q, k, v, do, km, mask


def _reference(c, q, k, v, do, mask, dtype=None):
    """Oracle output, gradients, weights and the statistics the forward saves: per row the maximum of the base-2 logits after the
    'masked logits are SET to -1e9' rule, and 1 / sum of 2^(logit - maximum)."""
    dtype = dtype or (np.float32 if c.mask == "allpad" else np.float64)
    qs, ks, vs = (_split(x, c.H).astype(dtype) for x in (q, k, v))
    o, a, cache = oracle.sdpa_fwd(qs, ks, vs, mask.astype(dtype))
    dq, dk, dv = oracle.sdpa_bwd(_split(do, c.H).astype(dtype), cache)
    s2 = (_split(q, c.H) @ np.swapaxes(_split(k, c.H), -1, -2)) * (LOG2E / np.sqrt(c.dh))
    s2 = np.where(np.broadcast_to(mask, s2.shape) > 0, -1e9, s2)
    mx = s2.max(-1)
    rinv = 1.0 / np.exp2(s2 - mx[..., None]).sum(-1)
    return _merge(o), (_merge(dq), _merge(dk), _merge(dv)), a, mx, rinv


def _hold_stats(kernel, stats, mx, rinv):
    got = stats.cpu().numpy().astype(np.float64)
    dead = mx == -1e9                                         # rows without a visible key: the maximum is the mask value itself
    assert np.array_equal(got[..., 0][dead], mx[dead])
    if (~dead).any():
        _hold(kernel, "row-max", got[..., 0][~dead], mx[~dead], FWD_BAR)
    rel = np.abs(got[..., 1] / rinv - 1.0).max()              # every row by itself: a backward kernel scales that row with it
    _WORST[kernel]["1/sum"] = max(_WORST[kernel].get("1/sum", 0.0), rel)
    assert rel <= FWD_BAR, "%s 1/sum: rel err %.3e" % (kernel, rel)


# ------------------------------------------------------------------ 1 + 2: every kernel of the dispatch against the oracle
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_every_dispatch_branch_matches_the_oracle(ops, c):
    default_split = _lib.default_precision() != F32
    if default_split:
        assert (c.fwd, c.bwd) == _dispatch(c.dh, c.prec, c.two_pass, c.Lq, c.Lk), "the case table names another kernel"
    q, k, v, do, km, mask = _inputs(c)
    want_o, want_g, _, mx, rinv = _reference(c, q, k, v, do, mask)
    kmd = _dev(km, torch.uint8) if km is not None else None
    qd, kd, vd, dod = _dev(q), _dev(k), _dev(v), _dev(do)
    with _Profiled() as prof:
        o, stats = ops.attention_fwd(qd, kd, vd, c.H, key_mask=kmd, causal=c.causal, precision=c.prec)
        g = ops.attention_bwd(qd, kd, vd, o, dod, stats, c.H, key_mask=kmd, causal=c.causal, precision=c.prec, two_pass=c.two_pass)
    if default_split:
        assert prof.tags == [_TAGS[c.fwd], _TAGS[c.bwd]], prof.tags
    _hold(c.fwd, "O", o, want_o, FWD_BAR)
    _hold_stats(c.fwd, stats, mx, rinv)
    for got, want, name in zip(g, want_g, ("dQ", "dK", "dV")):
        _hold(c.bwd, name, got, want, BWD_BAR, FLOOR)


# ------------------------------------------------------------------ 2: the two entry points of the builders front-end
_ROWSUM_BAR = 2e-6    # |sum of a row of weights - 1|: the kernels normalise e_i with the rounded 1 / sum(e_i) of the SAME e_i, so the
                      # exponential's error cancels; left are <= 22 fp32 additions of the sum (16 per lane, 6 across the wave), the
                      # division and one product per weight: 24 x 2^-24 = 1.43e-6


@pytest.mark.parametrize("dh,Lq,Lk,causal,kind", [(16, 37, 53, False, "pad"), (16, 209, 209, True, "pad"), (32, 65, 200, False, "allpad"),
                                                  (24, 63, 65, False, "hole"), (80, 64, 64, True, "none"), (8, 5, 1024, False, "pad")])
def test_attention_weights_entry_point(ops, dh, Lq, Lk, causal, kind):
    c = _c("skf_attention_weights", None, dh, None, False, causal, kind, Lq, Lk, B=3, H=2)
    q, k, v, do, km, mask = _inputs(c)
    want = _reference(c, q, k, v, do, mask)[2]
    w = ops.attention_weights(_dev(q), _dev(k), c.H, key_mask=_dev(km, torch.uint8) if km is not None else None, causal=causal)
    assert w.shape == (c.B, c.H, Lq, Lk)
    assert float((w.double().sum(-1) - 1.0).abs().max()) <= _ROWSUM_BAR
    _hold(c.fwd, "weights", w, want, FWD_BAR)


def _float_mask_reference(q, k, v, mask, H, dtype):
    qs, ks, vs = (_split(x, H).astype(dtype) for x in (q, k, v))
    logits = (qs @ np.swapaxes(ks, -1, -2)) / np.sqrt(np.asarray(ks.shape[-1], dtype))
    if mask is not None:
        logits = logits + mask.astype(dtype) * dtype(-1e9)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    return _merge(w @ vs), w


@pytest.mark.parametrize("dh", [16, 24], ids=["mfma_head_size", "other_head_size"])
@pytest.mark.parametrize("shape", ["B11Lk", "11LqLk", "BHLqLk", "B11Lk_all_masked_sample", "none"])
@pytest.mark.parametrize("return_weights", [False, True])
def test_attention_fwd_float_mask_entry_point(ops, dh, shape, return_weights):
    """softmax(q.k / sqrt(dh) + mask * -1e9) . v with the mask ADDED: 0.5 lowers a logit by 5e8, so the key vanishes beside an unmasked
    one.  A row that holds only 0.5s, or only 1.0s, has uniform weights: in fp32 the logit rounds away beside -5e8 like beside -1e9
    (float32 reference for the cases with such rows)."""
    B, H, Lq, Lk = 3, 2, 37, 65
    rng = np.random.RandomState(dh + len(shape))
    q, k, v = rng.randn(B, Lq, H * dh), rng.randn(B, Lk, H * dh), rng.randn(B, Lk, H * dh)
    dtype, mask = np.float64, None
    if shape != "none":
        dims = {"B11Lk": (B, 1, 1, Lk), "11LqLk": (1, 1, Lq, Lk), "BHLqLk": (B, H, Lq, Lk), "B11Lk_all_masked_sample": (B, 1, 1, Lk)}[shape]
        mask = rng.choice([0.0, 0.0, 0.5, 1.0], size=dims).astype(np.float32)
        mask[..., 3] = 0.0                                   # every row keeps one unmasked key ...
        if shape == "B11Lk_all_masked_sample":
            mask[1] = 1.0                                    # ... but this sample: no key at all
            dtype = np.float32
        if shape == "BHLqLk":
            mask[0, 1, 5, :] = 0.5                           # a row of equal non-binary values
            dtype = np.float32
    want_o, want_w = _float_mask_reference(q, k, v, mask, H, dtype)
    o, w = ops.attention_fwd_float_mask(_dev(q), _dev(k), _dev(v), H, mask=None if mask is None else _dev(mask), return_weights=return_weights)
    _hold("skf_attention_fwd_float_mask", "O", o, want_o, FWD_BAR)
    assert (w is not None) == return_weights
    if return_weights:
        assert float((w.double().sum(-1) - 1.0).abs().max()) <= _ROWSUM_BAR
        _hold("skf_attention_fwd_float_mask", "weights", w, want_w, FWD_BAR)


# ------------------------------------------------------------------ 3: properties of every backward kernel
Rep = collections.namedtuple("Rep", "bwd dh prec two_pass Lq Lk")
REPS = [Rep(BWD3, 16, None, False, 100, 128), Rep(B16, 16, None, False, 300, 209), Rep(B16 + " shared tile", 16, F32, False, 100, 200),
        Rep(B2_16, 16, None, True, 512, 512), Rep(B2_32, 32, None, False, 224, 255), Rep(B32, 32, None, False, 257, 100),
        Rep(B32 + " shared tile", 32, F32, False, 209, 72), Rep(B64, 64, None, False, 209, 273), Rep(BANY, 24, None, False, 65, 200)]
_rep_id = lambda r: r.bwd.replace(" ", "_")


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def _device_case(r, causal, B, H, seed):
    Lk = r.Lq if causal else r.Lk
    d = H * r.dh
    q, k, v, do = _rand((B, r.Lq, d), seed), _rand((B, Lk, d), seed + 1), _rand((B, Lk, d), seed + 2), _rand((B, r.Lq, d), seed + 3)
    lens = np.random.RandomState(seed).randint(1, Lk + 1, size=B)
    lens[0] = Lk
    km = torch.as_tensor(np.arange(Lk)[None, :] >= lens[:, None]).to(torch.uint8).cuda()
    return q, k, v, do, km, Lk


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("r", REPS, ids=_rep_id)
def test_live_query_lengths_change_no_bit(ops, r, causal):
    """dO is zero behind each sample's live length: the call with the length list returns the bits of the call without it, and dQ
    behind the live length is exactly zero.  Lengths 0 and Lq included; at Lq = 512 one sample's only extra live row sits in the
    32nd query tile (bit 31 of the two-pass kernel's live-tile word)."""
    B, H = 4, 2
    q, k, v, do, km, Lk = _device_case(r, causal, B, H, seed=31 + r.dh)
    rng = np.random.RandomState(r.Lq + r.dh)
    live = np.array([0, r.Lq, 16 * ((r.Lq - 1) // 16) + 1, rng.randint(1, r.Lq)], np.int32)
    do = do * (torch.arange(r.Lq, device="cuda")[None, :, None] < torch.as_tensor(live).cuda()[:, None, None])
    o, st = ops.attention_fwd(q, k, v, H, key_mask=km, causal=causal, precision=r.prec)
    kw = dict(key_mask=km, causal=causal, precision=r.prec, two_pass=r.two_pass)
    a = ops.attention_bwd(q, k, v, o, do, st, H, **kw)
    b = ops.attention_bwd(q, k, v, o, do, st, H, q_live_len=torch.as_tensor(live).cuda(), **kw)
    for x, y, n in zip(a, b, ("dQ", "dK", "dV")):
        assert torch.equal(x, y), n
    for s in range(B):
        assert float(b[0][s, live[s]:].abs().sum()) == 0.0, s
    assert float(b[0][1].abs().max()) > 0.0 and float(b[1][1].abs().max()) > 0.0


ORDERED = [  # (dh, precision, Lq, Lk, causal): forward <16,32,true>, <16,32,false>, <32,32>, <32,13>, <64,32>, <64,13>; backward one-pass
             # dh 16 (twice), attn_bwd2<dh32>, one-pass dh 32 and dh 64 (twice)
    (16, None, 300, 257, False), (16, F32, 257, 209, False), (16, None, 300, 300, True), (32, None, 200, 224, False),
    (32, F32, 100, 72, False), (32, None, 257, 257, True), (64, None, 100, 273, False), (64, None, 53, 37, False)]


@pytest.mark.parametrize("dh,prec,Lq,Lk,causal", ORDERED)
def test_sample_order_changes_no_bit(ops, dh, prec, Lq, Lk, causal):
    """B = 8, H = 4: the (sample, head) workgroups dealt from a sorted sample list and from a random permutation compute the bits of the
    plain numbering, forward (output and statistics) and backward."""
    B, H = 8, 4
    r = Rep("", dh, prec, False, Lq, Lk)
    q, k, v, do, km, Lk = _device_case(r, causal, B, H, seed=77 + dh + Lq)
    live = torch.as_tensor(np.random.RandomState(Lq).randint(0, Lq + 1, size=B).astype(np.int32)).cuda()
    do = do * (torch.arange(Lq, device="cuda")[None, :, None] < live[:, None, None])
    kw = dict(key_mask=km, causal=causal, precision=prec)
    o, st = ops.attention_fwd(q, k, v, H, **kw)
    g = ops.attention_bwd(q, k, v, o, do, st, H, q_live_len=live, **kw)
    perm = torch.as_tensor(np.random.RandomState(dh + Lk).permutation(B).astype(np.int32)).cuda()
    for order in (ops.sample_order(km, None), perm):
        o2, st2 = ops.attention_fwd(q, k, v, H, sample_order=order, **kw)
        assert torch.equal(o2, o) and torch.equal(st2, st)
        g2 = ops.attention_bwd(q, k, v, o, do, st, H, q_live_len=live, sample_order=order, **kw)
        for x, y, n in zip(g, g2, ("dQ", "dK", "dV")):
            assert torch.equal(x, y), n


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("r", REPS, ids=_rep_id)
def test_strided_operands_change_no_bit(ops, r, causal):
    """q, k, v as column slices of one (B, L, 3d) projection buffer (self-attention) or q alone and k, v of a (B, Lk, 2d) buffer
    (cross-attention), dO as a slice of a wider buffer - the way the train step passes them: the bits of the contiguous call."""
    B, H = 2, 2
    q, k, v, do, km, Lk = _device_case(r, causal, B, H, seed=55 + r.dh)
    d = H * r.dh
    if Lk == r.Lq:
        buf = torch.cat([q, k, v], dim=-1)
        qs, ks, vs = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    else:
        buf = torch.cat([k, v], dim=-1)
        qs, ks, vs = torch.cat([q, q], dim=-1)[..., d:], buf[..., :d], buf[..., d:]
    dos = torch.cat([do[..., :4], do, do[..., :4]], dim=-1)[..., 4:4 + d]
    assert not qs.is_contiguous() and not ks.is_contiguous() and not dos.is_contiguous()
    kw = dict(key_mask=km, causal=causal, precision=r.prec)
    o, st = ops.attention_fwd(q, k, v, H, **kw)
    o2, st2 = ops.attention_fwd(qs, ks, vs, H, **kw)
    assert torch.equal(o, o2) and torch.equal(st, st2)
    g = ops.attention_bwd(q, k, v, o, do, st, H, two_pass=r.two_pass, **kw)
    g2 = ops.attention_bwd(qs, ks, vs, o, dos, st, H, two_pass=r.two_pass, **kw)
    for x, y, n in zip(g, g2, ("dQ", "dK", "dV")):
        assert torch.equal(x, y), n


_SENTINEL = 0x7FC0DEAD          # a quiet NaN no kernel computes
_PITCH_PAD, _GUARD_ROWS = 4, 3


def _guarded(rows, cols):
    """A (rows, cols) view with row pitch cols + 4 inside a sentinel-filled buffer with guard rows on both sides."""
    buf = torch.full((rows + 2 * _GUARD_ROWS, cols + _PITCH_PAD), _SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[_GUARD_ROWS:_GUARD_ROWS + rows, :cols].view(torch.float32)


def _check_guarded(buf, rows, cols, name, written=True):
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[_GUARD_ROWS:_GUARD_ROWS + rows, :cols] = True
    hit = buf == _SENTINEL
    assert bool(hit[~inside].all()), name + ": a write outside the tensor's rows / columns"
    if written:
        assert not bool(hit[inside].any()), name + ": elements of the tensor were left unwritten"
    else:
        assert bool(hit[inside].all()), name + ": a refused call wrote output"


def _raw_fwd(q, k, v, km, causal, B, H, Lq, Lk, dh, o, ldo, stats, prec, ldq=None):
    _lib.call("skf_attention_fwd_ordered", q.data_ptr(), q.stride(1) if ldq is None else ldq, k.data_ptr(), k.stride(1), v.data_ptr(),
              v.stride(1), km.data_ptr() if km is not None else None, km.stride(0) if km is not None else 0, int(causal), B, H, Lq, Lk, dh,
              o.data_ptr(), ldo, stats.data_ptr(), prec, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _raw_bwd(q, k, v, o, ldo, do, stats, km, causal, B, H, Lq, Lk, dh, dq, dk, dv, ld, prec, live=None):
    _lib.call("skf_attention_bwd_ordered", q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(), v.stride(1), o.data_ptr(), ldo,
              do.data_ptr(), do.stride(1), stats.data_ptr(), km.data_ptr() if km is not None else None, km.stride(0) if km is not None else 0,
              int(causal), B, H, Lq, Lk, dh, dq.data_ptr(), ld, dk.data_ptr(), ld, dv.data_ptr(), ld, prec,
              live.data_ptr() if live is not None else None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _prec_arg(prec, two_pass=False):
    return (_lib.default_precision() if prec is None else prec) | (_lib.ATTN_TWO_PASS if two_pass else 0)


@pytest.mark.parametrize("dh,prec,two_pass,Lq,Lk,causal", [
    (16, None, False, 1, 17, False), (16, None, False, 17, 209, False), (16, None, False, 257, 257, True), (16, F32, False, 209, 257, False),
    (16, F32, False, 17, 17, True), (16, None, True, 257, 209, False), (16, None, True, 209, 209, True), (32, None, False, 209, 17, False),
    (32, None, False, 17, 257, False), (32, F32, False, 257, 1, False), (32, None, False, 257, 257, True), (64, None, False, 209, 257, False),
    (64, None, False, 1, 17, False), (64, None, False, 17, 17, True), (24, None, False, 17, 209, False), (40, None, False, 257, 257, True)])
def test_outputs_stay_inside_their_rows(ops, dh, prec, two_pass, Lq, Lk, causal):
    """O, dQ, dK, dV with a row pitch of d + 4 and the statistics, each between sentinel rows: after the calls every sentinel outside
    the tensors is untouched and none is left inside them (skipped key tiles and dead query tiles are still written, as zeros).
    Lengths that do not fill their last tile; padded keys; dO zero behind live lengths, the length list passed."""
    B, H = 3, 2
    d = H * dh
    r = Rep("", dh, prec, two_pass, Lq, Lk)
    q, k, v, do, km, Lk = _device_case(r, causal, B, H, seed=91 + dh + Lq)
    live = torch.as_tensor(np.array([Lq, 0, max(1, Lq // 2)], np.int32)).cuda()
    do = do * (torch.arange(Lq, device="cuda")[None, :, None] < live[:, None, None])
    obuf, o = _guarded(B * Lq, d)
    st_flat = torch.full(((B * H * Lq + 2 * _GUARD_ROWS) * 2,), _SENTINEL, dtype=torch.int32, device="cuda")     # (the statistics have no pitch)
    stats = st_flat[2 * _GUARD_ROWS:2 * _GUARD_ROWS + 2 * B * H * Lq].view(torch.float32)
    _raw_fwd(q, k, v, km, causal, B, H, Lq, Lk, dh, o, d + _PITCH_PAD, stats, _prec_arg(prec))
    torch.cuda.synchronize()
    _check_guarded(obuf, B * Lq, d, "O")
    hit = st_flat == _SENTINEL
    assert bool(hit[:2 * _GUARD_ROWS].all()) and bool(hit[-2 * _GUARD_ROWS:].all()) and not bool(hit[2 * _GUARD_ROWS:-2 * _GUARD_ROWS].any()), "stats"
    want_o, want_st = ops.attention_fwd(q, k, v, H, key_mask=km, causal=causal, precision=prec)
    assert torch.equal(o, want_o.view(B * Lq, d)) and torch.equal(stats, want_st.view(-1))
    (qb, dq), (kb, dk), (vb, dv) = _guarded(B * Lq, d), _guarded(B * Lk, d), _guarded(B * Lk, d)
    _raw_bwd(q, k, v, o, d + _PITCH_PAD, do, stats, km, causal, B, H, Lq, Lk, dh, dq, dk, dv, d + _PITCH_PAD, _prec_arg(prec, two_pass), live)
    torch.cuda.synchronize()
    for buf, rows, n in ((qb, B * Lq, "dQ"), (kb, B * Lk, "dK"), (vb, B * Lk, "dV")):
        _check_guarded(buf, rows, d, n)
    want = ops.attention_bwd(q, k, v, want_o, do, want_st, H, key_mask=km, causal=causal, precision=prec, two_pass=two_pass, q_live_len=live)
    for x, y, rows, n in zip((dq, dk, dv), want, (B * Lq, B * Lk, B * Lk), ("dQ", "dK", "dV")):
        assert torch.equal(x, y.view(rows, d)), n


# ------------------------------------------------------------------ 4: what does not fit is refused before any launch
# From fwd_smem / bwd_smem of skf_attention.hip against 160 KB = 40960 floats (n = length rounded up to whole 16-row tiles):
#   forward  dh 64: n (68 + 64 + 1 + 1/16) + 516 floats -> n <= 288;  dh 32: 69.0625 n + 260 -> 512 fits;  dh 16: fits
#   backward dh 64: 139 n + 9604 -> n <= 224;  dh 32: 75 n + 6788 -> n <= 448;  dh 16: 43 n + 7300 -> 512 fits
FWD, BWD = 1, 2
REFUSED = [  # (what, dh, precision, Lq, Lk, causal, ldq offset, the calls that are refused, message)
    ("dh 64 forward, one key tile over", 64, None, 16, 289, False, 0, FWD, "do not fit in LDS"),      # (its backward would fit: not called)
    ("dh 64 backward, one query tile over", 64, None, 225, 16, False, 0, BWD, "do not fit in LDS"),
    ("dh 32 one-pass backward, one query tile over", 32, F32, 449, 16, False, 0, BWD, "do not fit in LDS"),
    ("dh 32 split modes, one query tile over", 32, None, 449, 16, False, 0, BWD, "do not fit in LDS"),
    ("Lk = 513", 16, None, 16, 513, False, 0, FWD | BWD, "Lk > 512"),
    ("fallback, head size 132", 132, None, 16, 16, False, 0, FWD | BWD, "head dim"),
    ("fallback, 1025 keys", 24, None, 16, 1025, False, 0, FWD | BWD, "head dim"),
    ("fallback, 1025 queries", 24, None, 1025, 16, False, 0, FWD | BWD, "head dim"),
    ("look-ahead mask with Lq != Lk", 16, None, 32, 48, True, 0, FWD | BWD, "causal"),
    ("row stride 4k + 2", 16, None, 32, 32, False, 2, FWD | BWD, "multiples of 4"),
]


@pytest.mark.parametrize("what,dh,prec,Lq,Lk,causal,ld_off,refused,message", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_launch_limits_are_refused_and_nothing_is_written(what, dh, prec, Lq, Lk, causal, ld_off, refused, message):
    """Each call returns an error through the ABI before it launches anything: _lib.call raises with the skf_last_error text and the
    sentinel-filled outputs keep every sentinel.  (Where only the backward is refused the forward of the shape runs first.)"""
    B, H = 1, 1
    d = H * dh
    q, k, v, do = (torch.zeros(B, n, d, device="cuda") for n in (Lq, Lk, Lk, Lq))
    obuf, o = _guarded(B * Lq, d)
    sbuf, st = _guarded(B * H * Lq, 2)
    fwd = lambda out, stats: _raw_fwd(q, k, v, None, causal, B, H, Lq, Lk, dh, out, d + _PITCH_PAD, stats, _prec_arg(prec),
                                      ldq=d + ld_off if ld_off else None)
    stats = torch.zeros(B * H * Lq * 2, device="cuda")
    if refused & FWD:
        with pytest.raises(_lib.SkfError, match=message):
            fwd(o, st)          # (never launched: the pitch of st does not matter)
        torch.cuda.synchronize()
        _check_guarded(obuf, B * Lq, d, "O", written=False)
        _check_guarded(sbuf, B * H * Lq, 2, "stats", written=False)
    else:
        fwd(o, stats)
    if not refused & BWD:
        return
    (qb, dq), (kb, dk), (vb, dv) = _guarded(B * Lq, d), _guarded(B * Lk, d), _guarded(B * Lk, d)
    with pytest.raises(_lib.SkfError, match=message):
        _lib.call("skf_attention_bwd_ordered", q.data_ptr(), d + ld_off, k.data_ptr(), d, v.data_ptr(), d, o.data_ptr(), d + _PITCH_PAD,
                  do.data_ptr(), d, stats.data_ptr(), None, 0, int(causal), B, H, Lq, Lk, dh, dq.data_ptr(), d + _PITCH_PAD, dk.data_ptr(),
                  d + _PITCH_PAD, dv.data_ptr(), d + _PITCH_PAD, _prec_arg(prec), None, None,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for buf, rows, n in ((qb, B * Lq, "dQ"), (kb, B * Lk, "dK"), (vb, B * Lk, "dV")):
        _check_guarded(buf, rows, d, n, written=False)
