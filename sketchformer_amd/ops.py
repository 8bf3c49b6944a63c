"""Thin torch-tensor front-ends over the C ABI (one function per kernel family).

PyTorch only owns the device memory and the stream; every function checks
dtype / device / contiguity, passes raw pointers to libskf.so and raises
``SkfError`` on failure.  No CPU path exists.
"""
import ctypes as C

import torch

from . import _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.SkfError("sketchformer_amd ops need CUDA(HIP) tensors; got a CPU tensor (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _prec(precision):
    return _lib.default_precision() if precision is None else int(precision)


def _f32(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32" % name)
    if t.stride(-1) != 1:
        raise ValueError("%s must have a unit innermost stride" % name)
    return t


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _workspace_for(fn, device, *sizes):
    """The workspace of one call: ask the library's `fn` (a *_workspace_bytes) for these sizes and allocate that -> (ws, nbytes)."""
    nbytes = getattr(_lib.load(), fn)(*sizes)
    return _ws(nbytes, device), nbytes


def _ragged_offsets(offsets, rows, who, names=("offsets", "N", "flat", "sketch"), limit=True):
    """`offsets` (N + 1) int64 beside the (P, .) tensor `rows` -> (P, N).  names: the offsets, their count, the rows and one item in
    the texts; limit=False leaves P < 2^31 to the library (SkfError)."""
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.device != rows.device:
        raise TypeError("%s must be a contiguous int64 tensor of shape (%s + 1,) on the device of %s" % names[:3])
    P, N = rows.shape[0], offsets.shape[0] - 1
    if N < 1 or P < 1:
        raise ValueError("%s needs at least one %s and one point" % (who, names[3]))
    if limit and P >= 1 << 31:
        raise ValueError("%s takes fewer than 2^31 points" % who)
    return P, N


def _ragged(flat, offsets, who, limit=True):
    """The checks of a ragged batch of sketches, flat (P, 3) float32 + offsets (N + 1) int64, for the operation `who` -> (P, N)."""
    _p(flat); _p(offsets)                                        # CPU tensors: SkfError before anything is allocated
    if flat.dtype != torch.float32 or flat.dim() != 2 or flat.shape[1] != 3 or not flat.is_contiguous():
        raise TypeError("flat must be a contiguous float32 tensor of shape (P, 3)")
    return _ragged_offsets(offsets, flat, who, limit=limit)


def _compacted(out_flat, out_offsets):
    """-> (the P' = out_offsets[N] rows in use, the offsets); reading P' is one small device-to-host copy that waits for the stream."""
    kept = int(out_offsets[-1].item())
    return out_flat[:kept], out_offsets


def _centers(centers, beside=None):
    """The dictionary: centers (K, 2) float64, contiguous and, given beside = (tensor, its name), on that tensor's device -> K."""
    _p(centers)
    if centers.dtype != torch.float64 or centers.dim() != 2 or centers.shape[1] != 2 or not centers.is_contiguous() \
            or (beside is not None and centers.device != beside[0].device):
        raise TypeError("centers must be a contiguous float64 tensor of shape (K, 2)" + (" on the device of %s" % beside[1] if beside else ""))
    return centers.shape[0]


def new_step_state(device, iterations=0):
    """Device-resident per-step scalars {int64 iterations; f32 lr, alpha; u32 drop_key, micro}."""
    n = _lib.load().skf_step_state_bytes()
    st = torch.zeros(n // 8 + 1, dtype=torch.int64, device=device)
    st[0] = iterations
    return st


def step_prologue(state, schedule=0, p0=128.0, p1=5000 ** -1.5, p2=0.0, p3=0.0, beta1=0.9, beta2=0.98, seed=0):
    _lib.call("skf_step_prologue", _p(state), schedule, p0, p1, p2, p3, beta1, beta2, seed, _stream())


def step_epilogue(state):
    _lib.call("skf_step_epilogue", _p(state), _stream())


def read_step_state(state):
    """-> dict(iterations, lr, alpha, drop_key, micro) (host sync)."""
    raw = state.cpu().numpy().tobytes()
    import struct
    it, lr, alpha, key, micro = struct.unpack("<qffII", raw[:24])
    return {"iterations": it, "lr": lr, "alpha": alpha, "drop_key": key, "micro": micro}


def step_drop_key(seed, iterations, micro=0):
    """The dropout key the prologue writes for (seed, iterations, micro) (host only; skf_step_drop_key)."""
    return int(_lib.load().skf_step_drop_key(int(seed) & 0xffffffff, int(iterations), int(micro)))


def grad_accumulate(dst, a, b=None, state=None, micro_op=0):
    """dst = a + b (dst = a with b None) over flat float32 tensors of one size, on the current stream; dst may be a or b
    (skf_grad_accumulate: one fp32 add per element, the bits of torch's a + b).  micro_op: _lib.MICRO_KEEP / MICRO_NEXT / MICRO_ZERO on
    the `micro` word of the step state ``state`` (needed unless MICRO_KEEP).  Pointers that are not 16-byte aligned are refused by
    the library (SkfError, rc = SKF_EINVAL)."""
    for t, name in ((dst, "dst"), (a, "a"), (b, "b")):
        if t is None and name == "b":
            continue
        _p(t)
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.device != dst.device:
            raise TypeError("%s must be a contiguous 1-D float32 tensor on the device of dst" % name)
        if t.numel() != dst.numel():
            raise ValueError("dst, a and b must have the same number of elements")
    if micro_op not in (_lib.MICRO_KEEP, _lib.MICRO_NEXT, _lib.MICRO_ZERO):
        raise ValueError("micro_op must be 0 (leave the counter), 1 (micro += 1) or 2 (micro = 0)")
    if micro_op != _lib.MICRO_KEEP and state is None:
        raise ValueError("a micro_op that moves the counter needs the step state")
    _lib.call("skf_grad_accumulate", _p(dst), _p(a), _p(b), dst.numel(), _p(state), int(micro_op), _stream())
    return dst


def _flat_f32_pair(a, b, na, nb):
    for t, name in ((a, na), (b, nb)):
        _p(t)
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.device != a.device:
            raise TypeError("%s must be a contiguous 1-D float32 tensor on the device of %s" % (name, na))
        if t.numel() != a.numel():
            raise ValueError("%s and %s must have the same number of elements" % (na, nb))


def ema_decay_at(decay, num_updates=False, iterations=0):
    """The decay an averaging update uses at ``iterations`` (host only; skf_ema_decay_at): ``decay``, or with ``num_updates``
    min(decay, (1 + n) / (10 + n)) for n = float32(iterations), every operation in float32 - the expression the kernel evaluates."""
    return float(_lib.load().skf_ema_decay_at(float(decay), int(bool(num_updates)), int(iterations)))


def ema_update(shadow, w, decay, num_updates=False, state=None, skip=None):
    """shadow -= (shadow - w) * (1 - d) over flat float32 tensors of one size, on the current stream (skf_ema_update: three fp32
    operations per element, each rounded once - TensorFlow's assign_moving_average).  d = ``decay``, or with ``num_updates``
    min(decay, (1 + n) / (10 + n)) with n = the `iterations` word of the step state ``state``, read by the kernel.  ``skip``: a device
    tensor of 4-byte words (None = never); with skip[0] != 0 nothing is written.  Only ``shadow`` is written.  Pointers that are not
    16-byte aligned, overlapping operands and a decay outside (0, 1) are refused by the library (SkfError, rc = SKF_EINVAL)."""
    _flat_f32_pair(shadow, w, "shadow", "w")
    if num_updates and state is None:
        raise ValueError("num_updates reads `iterations`: it needs the step state")
    if skip is not None:
        _p(skip)
        if skip.element_size() != 4 or skip.numel() < 1 or skip.device != shadow.device:
            raise TypeError("skip must be a tensor of 4-byte words on the device of shadow")
    _lib.call("skf_ema_update", _p(shadow), _p(w), shadow.numel(), float(decay), int(bool(num_updates)), _p(state), _p(skip), _stream())
    return shadow


def buffer_swap(a, b):
    """Exchange the contents of two flat float32 tensors of one size in place, bit for bit (NaN payloads survive), on the current
    stream (skf_buffer_swap).  The same tensor twice, overlapping views and pointers that are not 16-byte aligned are refused by the
    library (SkfError, rc = SKF_EINVAL)."""
    _flat_f32_pair(a, b, "a", "b")
    _lib.call("skf_buffer_swap", _p(a), _p(b), a.numel(), _stream())


def target_live_len(tar, Ld):
    """(B, >= Ld + 1) int64 target tokens -> int32 (B,): 1 + last decoder row t < Ld trained on a non-PAD token tar[b, t+1]."""
    assert tar.dtype == torch.int64 and tar.dim() == 2 and tar.shape[1] > Ld
    out = torch.empty(tar.shape[0], dtype=torch.int32, device=tar.device)
    _lib.call("skf_target_live_len", _p(tar), tar.stride(0), tar.shape[0], Ld, _p(out), _stream())
    return out


def row_blocks(live_len, rows_per_sample, granule):
    """{n_live, n_blocks, live block ids, dead block ids} (int32) over `granule`-row blocks of the (B * rows_per_sample) rows."""
    B = live_len.shape[0]
    n = _lib.load().skf_row_blocks_bytes(B * rows_per_sample, granule) // 4
    out = torch.empty(n, dtype=torch.int32, device=live_len.device)
    _lib.call("skf_row_blocks_build", _p(live_len), B, rows_per_sample, granule, _p(out), _stream())
    return out


def relu_bits(M, N, K, device, precision=None):
    """Zeroed sign-bit buffer for gemm(..., relu_bits_out= / relu_bits_in=), or None when the shape has no such path."""
    n = _lib.load().skf_gemm_relu_bits_bytes(M, N, K, _prec(precision))
    return torch.zeros(n // 8, dtype=torch.int64, device=device) if n else None


def gemm(a, b, a_kcontig=True, b_kcontig=False, bias=None, act=0, relu_src=None, out=None, accumulate=False,
         splits=1, bias_grad=None, precision=None, row_blocks=None, row_block_rows=0, relu_bits_out=None, relu_bits_in=None):
    """C[M,N] (+)= opA(a) . opB(b).  a: [M,K] (a_kcontig) or [K,M]; b: [K,N] or [N,K] (b_kcontig).
    precision: SKF_PREC_* (0 fp32 MFMA, 6 bf16x6, 3 bf16x3); None = _lib.default_precision().
    row_blocks: list from ``row_blocks()`` - dgrad form with 16-row blocks (dead rows of a are zero), or the weight
    gradient (splits > 1 / bias_grad) with 32-row blocks over the contraction rows."""
    _f32(a, "a"); _f32(b, "b")
    M, K = (a.shape[0], a.shape[1]) if a_kcontig else (a.shape[1], a.shape[0])
    N = b.shape[0] if b_kcontig else b.shape[1]
    assert (b.shape[1] if b_kcontig else b.shape[0]) == K, "inner dimensions differ"
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    ws = None
    wsb = 0
    if splits > 1 or bias_grad is not None:
        wsb = _lib.load().skf_gemm_workspace_bytes(M, N, K, splits, 1)
        ws = _ws(wsb, a.device)
    if row_blocks is not None and (splits > 1 or bias_grad is not None):
        # the weight gradient in its two phases: partial tiles over the live contraction blocks, then the slab reduction
        assert not a_kcontig and not b_kcontig
        used = C.c_int(0)
        _lib.call("skf_gemm_wgrad_partial_rows", M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), splits,
                  int(bias_grad is not None), _p(ws), wsb, C.byref(used), _prec(precision), _p(row_blocks), row_block_rows, _stream())
        _lib.call("skf_splitk_reduce", _p(ws), used.value, M, N, _p(out), out.stride(0), int(accumulate), _p(bias_grad), 0, _stream())
        return out
    if relu_bits_out is not None or relu_bits_in is not None:
        _lib.call("skf_gemm_f32_bits", int(a_kcontig), int(b_kcontig), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0),
                  _p(out), out.stride(0), _p(bias), act, _p(relu_src), relu_src.stride(0) if relu_src is not None else 0,
                  int(accumulate), splits, _p(bias_grad), 0, _p(ws), wsb, _prec(precision), _p(row_blocks), row_block_rows,
                  _p(relu_bits_out), _p(relu_bits_in), _stream())
        return out
    if row_blocks is not None:
        _lib.call("skf_gemm_f32_rows", int(a_kcontig), int(b_kcontig), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0),
                  _p(out), out.stride(0), _p(bias), act, _p(relu_src), relu_src.stride(0) if relu_src is not None else 0,
                  int(accumulate), splits, _p(bias_grad), 0, _p(ws), wsb, _prec(precision), _p(row_blocks), row_block_rows, _stream())
        return out
    _lib.call("skf_gemm_f32", int(a_kcontig), int(b_kcontig), M, N, K, _p(a), a.stride(0), _p(b), b.stride(0),
              _p(out), out.stride(0), _p(bias), act, _p(relu_src), relu_src.stride(0) if relu_src is not None else 0,
              int(accumulate), splits, _p(bias_grad), 0, _p(ws), wsb, _prec(precision), _stream())
    return out


def sample_order(mask_a=None, mask_b=None):
    """uint8 padding masks (B, La) / (B, Lb), 1 = padded -> int32 (B,): the samples by unmasked positions, most first (skf_sample_order)."""
    m = mask_a if mask_a is not None else mask_b
    out = torch.empty(m.shape[0], dtype=torch.int32, device=m.device)
    _lib.call("skf_sample_order", _p(mask_a), mask_a.stride(0) if mask_a is not None else 0, mask_a.shape[1] if mask_a is not None else 0,
              _p(mask_b), mask_b.stride(0) if mask_b is not None else 0, mask_b.shape[1] if mask_b is not None else 0, m.shape[0], _p(out),
              _stream())
    return out


def attention_fwd(q, k, v, num_heads, key_mask=None, causal=False, precision=None, sample_order=None):
    """q (B,Lq,d) k,v (B,Lk,d) views with unit inner stride -> o (B,Lq,d), stats (B,H,Lq,2).
    sample_order: optional int32 (B,) from ``sample_order`` - workgroup numbering only, never a result bit."""
    B, Lq, d = q.shape
    Lk = k.shape[1]
    o = torch.empty(B, Lq, d, dtype=torch.float32, device=q.device)
    stats = torch.empty(B, num_heads, Lq, 2, dtype=torch.float32, device=q.device)
    _lib.call("skf_attention_fwd_ordered", _p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(key_mask),
              key_mask.stride(0) if key_mask is not None else 0, int(causal), B, num_heads, Lq, Lk, d // num_heads,
              _p(o), o.stride(1), _p(stats), _prec(precision), _p(sample_order), _stream())
    return o, stats


def attention_weights(q, k, num_heads, key_mask=None, causal=False):
    """softmax(q.k/sqrt(dh) + mask*-1e9) as the (B,H,Lq,Lk) tensor builders/utils.py:105 returns; q (B,Lq,d), k (B,Lk,d) views."""
    B, Lq, d = q.shape
    Lk = k.shape[1]
    w = torch.empty(B, num_heads, Lq, Lk, dtype=torch.float32, device=q.device)
    _lib.call("skf_attention_weights", _p(q), q.stride(1), _p(k), k.stride(1), _p(key_mask),
              key_mask.stride(0) if key_mask is not None else 0, int(causal), B, num_heads, Lq, Lk, d // num_heads, _p(w), _stream())
    return w


def attention_fwd_float_mask(q, k, v, num_heads, mask=None, return_weights=False):
    """softmax(q.k/sqrt(dh) + mask * -1e9) . v for ANY float mask broadcastable to (B,H,Lq,Lk) (builders/utils.py:90-105);
    q (B,Lq,d), k/v (B,Lk,d) views -> (o (B,Lq,d), weights (B,H,Lq,Lk) or None).  skf_attention_fwd_float_mask."""
    B, Lq, d = q.shape
    Lk = k.shape[1]
    o = torch.empty(B, Lq, d, dtype=torch.float32, device=q.device)
    w = torch.empty(B, num_heads, Lq, Lk, dtype=torch.float32, device=q.device) if return_weights else None
    sb = sh = sq = 0
    if mask is not None:
        mask = torch.as_tensor(mask, device=q.device).detach().to(torch.float32)
        while mask.dim() < 4:
            mask = mask[None]
        if mask.stride(-1) != 1 and mask.shape[-1] != 1:
            mask = mask.contiguous()
        mask = torch.broadcast_to(mask, (B, num_heads, Lq, Lk))
        if mask.stride(-1) != 1:                 # a broadcast key axis: materialise (the kernel wants unit stride there)
            mask = mask.contiguous()
        sb, sh, sq = mask.stride(0), mask.stride(1), mask.stride(2)
    _lib.call("skf_attention_fwd_float_mask", _p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(mask), sb, sh, sq,
              B, num_heads, Lq, Lk, d // num_heads, _p(o), o.stride(1), _p(w), _stream())
    return o, w


def row_mean(a, b=None, mode=0):
    """mean over the last axis of a (mode 0), |a - b| (1) or (a - b)^2 (2) -> a.shape[:-1]  (skf_row_mean)"""
    a = torch.as_tensor(a).detach().to(device="cuda", dtype=torch.float32).contiguous()
    if b is not None:
        b = torch.as_tensor(b, device=a.device).detach().to(torch.float32).expand_as(a).contiguous()
    cols = a.shape[-1]
    out = torch.empty(a.shape[:-1], dtype=torch.float32, device=a.device)
    _lib.call("skf_row_mean", _p(a), _p(b), a.numel() // cols, cols, int(mode), _p(out), _stream())
    return out


def attention_decode(q, k, v, num_heads, n_keys=None, key_mask=None, key_limit=None, key_limit_all=0, step=None,
                     k_new=None, v_new=None, limit_from_step=False):
    """One query row per (sample, head): q (B,d), k/v (B,Lcap,d) cache views with unit inner stride, the first
    n_keys rows of each sample are used -> o (B,d)."""
    B, d = q.shape
    Lk = k.shape[1] if n_keys is None else int(n_keys)
    assert k.stride(0) == v.stride(0) and k.stride(1) == v.stride(1)
    o = torch.empty(B, d, dtype=torch.float32, device=q.device)
    _lib.call("skf_attention_decode", _p(q), q.stride(0), _p(k), _p(v), k.stride(1), k.stride(0), _p(key_mask),
              key_mask.stride(0) if key_mask is not None else 0, _p(key_limit), int(key_limit_all), B, num_heads, Lk,
              d // num_heads, _p(o), o.stride(0), _p(step), _p(k_new), _p(v_new), k_new.stride(0) if k_new is not None else 0,
              int(limit_from_step), _stream())
    return o


def attention_bwd(q, k, v, o, do, stats, num_heads, key_mask=None, causal=False, precision=None, q_live_len=None, two_pass=False,
                  sample_order=None):
    """q_live_len: optional int32 (B,) - query rows at or behind it have do == 0 exactly (``target_live_len``).
    two_pass: OR SKF_ATTN_TWO_PASS into the precision argument (the two-pass kernel of skf_attention_bwd2.hip also where the
    dispatch would take the one-pass kernel: head size 16)."""
    B, Lq, d = q.shape
    Lk = k.shape[1]
    dq = torch.full((B, Lq, d), float("nan"), dtype=torch.float32, device=q.device)
    dk = torch.empty(B, Lk, d, dtype=torch.float32, device=q.device)
    dv = torch.empty(B, Lk, d, dtype=torch.float32, device=q.device)
    _lib.call("skf_attention_bwd_ordered", _p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(o), o.stride(1),
              _p(do), do.stride(1), _p(stats), _p(key_mask), key_mask.stride(0) if key_mask is not None else 0,
              int(causal), B, num_heads, Lq, Lk, d // num_heads, _p(dq), dq.stride(1), _p(dk), dk.stride(1),
              _p(dv), dv.stride(1), _prec(precision) | (_lib.ATTN_TWO_PASS if two_pass else 0), _p(q_live_len), _p(sample_order), _stream())
    return dq, dk, dv


def padding_mask(tokens, L=None):
    B, ld = tokens.shape
    L = L or ld
    out = torch.empty(B, L, dtype=torch.uint8, device=tokens.device)
    _lib.call("skf_padding_mask", _p(tokens), ld, B, L, _p(out), _stream())
    return out


def embed_fwd(tokens, table, pos, L=None, rate=0.0, site=0, state=None):
    B, ld = tokens.shape
    L = L or ld
    V, d = table.shape
    out = torch.empty(B, L, d, dtype=torch.float32, device=table.device)
    _lib.call("skf_embed_fwd", _p(tokens), ld, B, L, _p(table), V, d, _p(pos), _p(out), rate, site, _p(state), _stream())
    return out


def embed_bwd(tokens, dx, vocab, L=None, rate=0.0, site=0, state=None):
    B, ld = tokens.shape
    L = L or ld
    d = dx.shape[-1]
    dtable = torch.zeros(vocab, d, dtype=torch.float32, device=dx.device)
    _lib.call("skf_embed_bwd", _p(tokens), ld, B, L, _p(dx), vocab, d, _p(dtable), rate, site, _p(state), _stream())
    return dtable


def embed_bwd_sorted(tokens, dx, vocab, L=None, rate=0.0, site=0, state=None, prefill=None):
    """The two-launch form (skf_embed_sort + skf_embed_bwd_sorted); dtable starts as `prefill` (garbage is fine: every row is
    written) to show that no pre-zeroed table is needed."""
    B, ld = tokens.shape
    L = L or ld
    d = dx.shape[-1]
    dtable = torch.full((vocab, d), float("nan") if prefill is None else prefill, dtype=torch.float32, device=dx.device)
    nbytes = _lib.load().skf_embed_sort_workspace_bytes(B, L, vocab)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dx.device)
    _lib.call("skf_embed_sort", _p(tokens), ld, B, L, vocab, _p(dtable), d, _p(ws), nbytes, _stream())
    _lib.call("skf_embed_bwd_sorted", _p(ws), B, L, _p(dx), vocab, d, _p(dtable), rate, site, _p(state), _stream())
    return dtable


def layernorm_residual_fwd(x, y, gamma, beta, rate=0.0, site=0, state=None):
    """-> out, z (= x + drop(y), written over a copy of y), stats."""
    d = x.shape[-1]
    rows = x.numel() // d
    z = y.clone()
    out = torch.empty_like(x)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    _lib.call("skf_layernorm_residual_fwd", _p(x), _p(z), _p(gamma), _p(beta), _p(out), _p(stats), rows, d, rate, site,
              _p(state), _stream())
    return out, z, stats


def gemm_ln_residual(a, w, bias, x, gamma, beta, rate=0.0, site=0, state=None, precision=None):
    """One launch: z = x + dropout(a . w + bias), out = LayerNorm(z) -> out, z, stats (skf_gemm_ln_residual_f32;
    K = N = 128 in a split-arithmetic mode only)."""
    _f32(a, "a"); _f32(w, "w"); _f32(x, "x")
    M, K = a.shape
    N = w.shape[1]
    z = torch.empty(M, N, dtype=torch.float32, device=a.device)
    out = torch.empty_like(z)
    stats = torch.empty(M, 2, dtype=torch.float32, device=a.device)
    _lib.call("skf_gemm_ln_residual_f32", M, N, K, _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(x), _p(gamma), _p(beta),
              _p(z), _p(out), _p(stats), rate, site, _p(state), _prec(precision), _stream())
    return out, z, stats


def ffn_fused_supported(M, d, dff, precision=None):
    return bool(_lib.load().skf_ffn_fused_supported(M, d, dff, _prec(precision)))


def ffn_weight_images(pairs, transpose, precision=None):
    """pairs: [(W1 [d, dff], W2 [dff, d]), ...] -> one uint8 tensor per pair holding the pre-split operand image
    (transpose=False: the forward's, True: the input gradient's); all pairs in ONE launch (skf_ffn_weight_images)."""
    n = len(pairs)
    d, dff = pairs[0][0].shape
    nbytes = _lib.load().skf_ffn_image_bytes(d, dff, _prec(precision))
    if not nbytes:
        raise _lib.SkfError("no fused feed-forward path for d=%d dff=%d" % (d, dff))
    imgs = [torch.empty(nbytes, dtype=torch.uint8, device=pairs[0][0].device) for _ in range(n)]
    PA = C.c_void_p * n
    IA = C.c_int * n
    for w1, w2 in pairs:
        _f32(w1, "W1"); _f32(w2, "W2")
    _lib.call("skf_ffn_weight_images", n, PA(*[w1.data_ptr() for w1, _ in pairs]), IA(*[w1.stride(0) for w1, _ in pairs]),
              PA(*[w2.data_ptr() for _, w2 in pairs]), IA(*[w2.stride(0) for _, w2 in pairs]), IA(*([int(bool(transpose))] * n)),
              PA(*[im.data_ptr() for im in imgs]), d, dff, _prec(precision), _stream())
    return imgs


def ffn_fused_fwd(x, image, b1, b2, gamma, beta, dff, rate=0.0, site=0, state=None, precision=None, proj=None):
    """One launch: h = relu(x.W1 + b1), z = x + dropout(h.W2 + b2), out = LayerNorm(z) -> out, z, stats, h, sign bits.
    proj = (image of Wp [d, n], bias [n]): also out . Wp + bias in the same launch -> (..., proj_out)."""
    _f32(x, "x")
    M, d = x.shape
    h = torch.empty(M, dff, dtype=torch.float32, device=x.device)
    nb = _lib.load().skf_ffn_relu_bits_bytes(M, d, dff, _prec(precision))
    bits = torch.zeros(max(nb // 8, 1), dtype=torch.int64, device=x.device)
    z = torch.empty_like(x)
    out = torch.empty_like(x)
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device)
    if proj is not None:
        pimg, pbias = proj
        po = torch.empty(M, pbias.numel(), dtype=torch.float32, device=x.device)
        _lib.call("skf_ffn_fused_fwd_proj_f32", M, d, dff, _p(x), _p(image), _p(b1), _p(b2), _p(h), _p(bits), _p(gamma), _p(beta),
                  _p(z), _p(out), _p(stats), rate, site, _p(state), _p(pimg), _p(pbias), pbias.numel(), _p(po), _prec(precision), _stream())
        return out, z, stats, h, bits, po
    _lib.call("skf_ffn_fused_fwd_f32", M, d, dff, _p(x), _p(image), _p(b1), _p(b2), _p(h), _p(bits), _p(gamma), _p(beta),
              _p(z), _p(out), _p(stats), rate, site, _p(state), _prec(precision), _stream())
    return out, z, stats, h, bits


def ffn_block_fwd(a, residual, pre, image, b1, b2, gamma, beta, dff, rate=0.0, pre_site=0, site=0, state=None, precision=None, proj=None):
    """The forward launch in its general form (skf_ffn_block_fwd_f32): pre = (image of Wo, bias, gamma1, beta1): the launch starts at the
    attention output `a` and forms z1 = residual + dropout(a.Wo + bo), x1 = LayerNorm(z1) in front of the feed-forward block
    -> dict(z1, x1, stats1, h, bits, z, out, stats[, proj_out])."""
    _f32(a, "a")
    M, d = a.shape
    dev = a.device
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)  # noqa: E731
    r = {"h": e(M, dff), "z": e(M, d), "out": e(M, d), "stats": e(M, 2), "z1": e(M, d), "x1": e(M, d), "stats1": e(M, 2)}
    nb = _lib.load().skf_ffn_relu_bits_bytes(M, d, dff, _prec(precision))
    r["bits"] = torch.zeros(max(nb // 8, 1), dtype=torch.int64, device=dev)
    pimg, pbias, pg, pb = pre
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    blk = _lib.SkfFfnBlockFwd(struct_size=C.sizeof(_lib.SkfFfnBlockFwd), M=M, d=d, dff=dff, precision=_prec(precision), x=P(a), image=P(image),
                              b1=P(b1), b2=P(b2), h=P(r["h"]), relu_bits_out=P(r["bits"]), gamma=P(gamma), beta=P(beta), z=P(r["z"]),
                              out=P(r["out"]), stats=P(r["stats"]), rate=rate, site=site, step_state=P(state), pre_image=P(pimg),
                              pre_bias=P(pbias), pre_residual=P(residual), pre_gamma=P(pg), pre_beta=P(pb), pre_z=P(r["z1"]), pre_out=P(r["x1"]),
                              pre_stats=P(r["stats1"]), pre_site=pre_site)
    if proj is not None:
        r["proj_out"] = e(M, proj[1].numel())
        blk.proj_image, blk.proj_bias, blk.proj_out, blk.proj_n = P(proj[0]), P(proj[1]), P(r["proj_out"]), proj[1].numel()
    _lib.call("skf_ffn_block_fwd_f32", C.byref(blk), _stream())
    return r


def attn_tail_proj(a, residual, pre, proj, rate=0.0, pre_site=0, state=None, precision=None):
    """skf_ffn_block_fwd_f32 without a feed-forward image: z1 = residual + dropout(a.Wo + bo), x1 = LayerNorm(z1), proj_out = x1.Wp + bp in
    one launch (pre = (image of Wo, bo, gamma, beta), proj = (image of Wp, bp)) -> dict(z1, x1, stats1, proj_out)."""
    _f32(a, "a")
    M, d = a.shape
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=a.device)  # noqa: E731
    r = {"z1": e(M, d), "x1": e(M, d), "stats1": e(M, 2), "proj_out": e(M, proj[1].numel())}
    pimg, pbias, pg, pb = pre
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    blk = _lib.SkfFfnBlockFwd(struct_size=C.sizeof(_lib.SkfFfnBlockFwd), M=M, d=d, dff=4 * d, precision=_prec(precision), x=P(a), rate=rate,
                              step_state=P(state), pre_image=P(pimg), pre_bias=P(pbias), pre_residual=P(residual), pre_gamma=P(pg), pre_beta=P(pb),
                              pre_z=P(r["z1"]), pre_out=P(r["x1"]), pre_stats=P(r["stats1"]), pre_site=pre_site, proj_image=P(proj[0]),
                              proj_bias=P(proj[1]), proj_out=P(r["proj_out"]), proj_n=proj[1].numel())
    _lib.call("skf_ffn_block_fwd_f32", C.byref(blk), _stream())
    return r


def ffn_fused_bwd(dy, image_t, bits, dff, dx=None, row_blocks=None, precision=None):
    """One launch: dh = (dy.W2^T) o relu'(h), dx (+)= dh.W1^T -> dh, dx (accumulated into `dx` when given)."""
    _f32(dy, "dy")
    M, d = dy.shape
    dh = torch.empty(M, dff, dtype=torch.float32, device=dy.device)
    acc = dx is not None
    if dx is None:
        dx = torch.empty_like(dy)
    _lib.call("skf_ffn_fused_bwd_f32", M, d, dff, _p(dy), _p(image_t), _p(bits), _p(dh), _p(dx), int(acc), _p(row_blocks),
              16 if row_blocks is not None else 0, _prec(precision), _stream())
    return dh, dx


def ffn_fused_bwd_ln(dout, z, stats, gamma, image_t, bits, dff, rate=0.0, site=0, state=None, row_blocks=None, precision=None):
    """One launch from the gradient of the closing LayerNorm's output: -> dy, dh, dx (= dz + dh.W1^T), dgamma, dbeta."""
    _f32(dout, "dout")
    M, d = dout.shape
    lib = _lib.load()
    n = lib.skf_ffn_fused_ln_partials(M)
    part = torch.empty(n, 2, d, dtype=torch.float32, device=dout.device)
    dy, dx = torch.empty_like(dout), torch.empty_like(dout)
    dh = torch.empty(M, dff, dtype=torch.float32, device=dout.device)
    _lib.call("skf_ffn_fused_bwd_ln_f32", M, d, dff, _p(dout), _p(z), _p(stats), _p(gamma), rate, site, _p(state), _p(image_t), _p(bits),
              _p(dy), _p(dh), _p(dx), _p(part), part.numel() * 4, _p(row_blocks), 16 if row_blocks is not None else 0, _prec(precision),
              _stream())
    g = part.sum(0)
    return dy, dh, dx, g[0], g[1]


def dense_weight_image(w, transpose, precision=None):
    """Pre-split MFMA operand image of B = w [K, N] (transpose=False) or w^T (w is [N, K]) - skf_dense_weight_images."""
    _f32(w, "w")
    K, N = (w.shape[1], w.shape[0]) if transpose else (w.shape[0], w.shape[1])
    nbytes = _lib.load().skf_dense_image_bytes(K, N, _prec(precision))
    if not nbytes:
        raise _lib.SkfError("no operand image for K=%d N=%d" % (K, N))
    img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    PA, IA = C.c_void_p * 1, C.c_int * 1
    _lib.call("skf_dense_weight_images", 1, PA(w.data_ptr()), IA(w.stride(0)), IA(int(bool(transpose))), IA(K), IA(N), PA(img.data_ptr()),
              _prec(precision), _stream())
    return img


def layernorm_bwd_dgrad(dout, z, stats, gamma, image_t, rate=0.0, site=0, state=None, row_blocks=None, precision=None, lead=None):
    """One launch: dz = LayerNorm'(dout), dy = dropout'(dz), da = dy . W^T -> dz, dy, da, dgamma, dbeta (skf_layernorm_bwd_dgrad_f32).
    lead = (rows a [M, d], transposed image of Wl): the LayerNorm output's gradient is dout + a . Wl^T (skf_layernorm_bwd_dgrad_lead_f32)."""
    _f32(dout, "dout")
    M, d = dout.shape
    n = _lib.load().skf_layernorm_bwd_dgrad_partials(M)
    part = torch.empty(n, 2, d, dtype=torch.float32, device=dout.device)
    dz, dy, da = torch.empty_like(dout), torch.empty_like(dout), torch.empty_like(dout)
    la, li = lead if lead is not None else (None, None)
    _lib.call("skf_layernorm_bwd_dgrad_lead_f32", M, d, _p(dout), _p(la), _p(li), _p(z), _p(stats), _p(gamma), rate, site, _p(state), _p(image_t),
              _p(dz), _p(dy), _p(da), _p(part), part.numel() * 4, _p(row_blocks), 16 if row_blocks is not None else 0, _prec(precision), _stream())
    g = part.sum(0)
    return dz, dy, da, g[0], g[1]


def layernorm_residual_bwd(dout, z, stats, gamma, rate=0.0, site=0, state=None):
    d = dout.shape[-1]
    rows = dout.numel() // d
    dz = torch.empty_like(dout)
    dy = torch.empty_like(dout) if rate > 0 else None
    dg = torch.empty(d, dtype=torch.float32, device=dout.device)
    db = torch.empty(d, dtype=torch.float32, device=dout.device)
    ws, wsb = _workspace_for("skf_layernorm_bwd_workspace_bytes", dout.device, rows, d)
    _lib.call("skf_layernorm_residual_bwd", _p(dout), _p(z), _p(stats), _p(gamma), _p(dz), _p(dy), _p(dg), _p(db), rows,
              d, rate, site, _p(state), _p(ws), wsb, _stream())
    return dz, (dy if dy is not None else dz), dg, db


def softmax_ce(logits, target, tgt_cols, tgt_off=0, mask_pad=False, scale=1.0, want_probs=False, write_grad=True):
    """In place: logits (rows, ncls) become the gradient.  target: int64 (B, tgt_ld)."""
    rows, ncls = logits.shape
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_hit = torch.empty(rows, dtype=torch.float32, device=logits.device)
    probs = torch.empty(rows, ncls, dtype=torch.float32, device=logits.device) if want_probs else None
    _lib.call("skf_softmax_ce", _p(logits), logits.stride(0), rows, ncls, _p(target), target.stride(0), tgt_cols, tgt_off,
              int(mask_pad), scale, _p(row_loss), _p(row_hit), _p(probs), int(write_grad), _stream())
    return row_loss, row_hit, probs


def pool_fwd(u, Vw, x):
    B, L, U = u.shape
    d = x.shape[-1]
    a = torch.empty(B, L, dtype=torch.float32, device=x.device)
    emb = torch.empty(B, d, dtype=torch.float32, device=x.device)
    _lib.call("skf_pool_fwd", _p(u), _p(Vw), _p(x), B, L, U, d, _p(a), _p(emb), _stream())
    return a, emb


def pool_bwd(u, Vw, x, a, demb):
    """-> dpre (overwrites a copy of u), dx_direct, dV."""
    B, L, U = u.shape
    d = x.shape[-1]
    dpre = u.clone()
    dx = torch.empty_like(x)
    dV = torch.empty(U, dtype=torch.float32, device=x.device)
    ws = _ws(B * U * 4, x.device)
    _lib.call("skf_pool_bwd", _p(dpre), _p(Vw), _p(x), _p(a), _p(demb), B, L, U, d, _p(dx), _p(dV), _p(ws), B * U * 4,
              _stream())
    return dpre, dx, dV


def expander_fwd(emb, w, bias):
    B, d = emb.shape
    L = w.numel()
    pre = torch.empty(B, L, d, dtype=torch.float32, device=emb.device)
    _lib.call("skf_expander_fwd", _p(emb), _p(w), _p(bias), B, L, d, _p(pre), _stream())
    return pre


def expander_bwd(dpre, emb, w):
    B, L, d = dpre.shape
    demb = torch.empty(B, d, dtype=torch.float32, device=emb.device)
    dw = torch.empty(L, dtype=torch.float32, device=emb.device)
    db = torch.empty(L, dtype=torch.float32, device=emb.device)
    ws = _ws(2 * B * L * 4, emb.device)
    _lib.call("skf_expander_bwd", _p(dpre), _p(emb), _p(w), B, L, d, _p(demb), 0, _p(dw), _p(db), _p(ws), 2 * B * L * 4,
              _stream())
    return demb, dw, db


def adam_step(w, g, m, v, state, grad_scale=1.0, beta1=0.9, beta2=0.98, eps=1e-9):
    _lib.call("skf_adam_step", _p(w), _p(g), _p(m), _p(v), w.numel(), _p(state), grad_scale, beta1, beta2, eps, _stream())


def sgd_momentum_step(w, g, velocity, state, grad_scale=1.0, momentum=0.9):
    _lib.call("skf_sgd_momentum_step", _p(w), _p(g), _p(velocity), w.numel(), _p(state), grad_scale, momentum, _stream())


# ---- gradient norms and clipping (include/skf.h: skf_segment_*, skf_adam_step_clipped)
CLIP_MODES = {"none": 0, "per_variable": 1, "global": 2}         # SKF_CLIP_*
SEGMENT_CHUNK = 16384                                            # SKF_SEGMENT_CHUNK


class SegmentPlan:
    """What ``segment_plan`` returns: the uploaded chunk table of one entry layout (``dev``, a uint8 tensor) and its counts."""
    __slots__ = ("dev", "n_entries", "n_chunks", "entries")

    def __init__(self, dev, n_entries, n_chunks, entries):
        self.dev, self.n_entries, self.n_chunks, self.entries = dev, n_entries, n_chunks, entries


def _entry_array(entries):
    arr = (_lib.SkfParamEntry * len(entries))()
    for a, e in zip(arr, entries):
        if isinstance(e, dict):
            e = (e["offset"], e["rows"], e["cols"], e["row_stride"])
        a.offset, a.rows, a.cols, a.row_stride = (int(x) for x in e)
    return arr


def segment_plan(entries, device):
    """The segment plan of an entry table, built on the host and uploaded once per layout.  entries: the dicts of
    ``engine.param_entries`` or (offset, rows, cols, row_stride) tuples, in floats; strided entries are read as strided views and
    the floats between entries are never read."""
    lib = _lib.load()
    arr = _entry_array(entries)
    n = len(entries)
    n_chunks = lib.skf_segment_plan_chunks(arr, n)
    if n_chunks < 0:
        _lib.check(n_chunks, "skf_segment_plan_chunks")
    nbytes = lib.skf_segment_plan_bytes(n, n_chunks)
    host = torch.zeros(nbytes, dtype=torch.uint8)
    _lib.call("skf_segment_plan_build", arr, n, C.c_void_p(host.data_ptr()), nbytes)
    return SegmentPlan(host.to(device), n, n_chunks, list(entries))


def new_segment_stats(plan):
    """The 8 + 2 E stats words of ``segment_norms`` as a float32 tensor: norms and counters 0, every scale 1."""
    st = torch.zeros(8 + 2 * plan.n_entries, dtype=torch.float32, device=plan.dev.device)
    st[1] = 1.0
    st[8 + plan.n_entries:] = 1.0
    return st


def segment_norms(flat, plan, grad_scale=1.0, mode="none", threshold=0.0, skip_nonfinite=False, stats=None, workspace=None):
    """Per-entry and global L2 norms of a flat float32 buffer, the clip scales and the skip decision: skf_segment_norms, two
    launches, deterministic.  mode: 'none' | 'per_variable' | 'global'.  Returns the stats tensor (layout in include/skf.h;
    ``read_segment_stats`` turns it into a dict): pass the same tensor again to keep its skipped total."""
    _f32(flat, "flat")
    if stats is None:
        stats = new_segment_stats(plan)
    nbytes = _lib.load().skf_segment_norms_workspace_bytes(plan.n_entries, plan.n_chunks)
    ws = _ws(nbytes + 256, flat.device) if workspace is None else workspace
    off = (-ws.data_ptr()) % 256
    _lib.call("skf_segment_norms", _p(flat), _p(plan.dev), plan.n_entries, plan.n_chunks, float(grad_scale), CLIP_MODES[mode],
              float(threshold), int(bool(skip_nonfinite)), C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _p(stats), _stream())
    return stats


def read_segment_stats(stats, n_entries=None):
    """The stats words on the host (one copy; waits for the stream) -> dict(global_norm, scale, nonfinite, skipped, skipped_total,
    norms (E,), scales (E,))."""
    raw = stats.detach().cpu().numpy()
    E = (len(raw) - 8) // 2 if n_entries is None else int(n_entries)
    words = raw[:8].view("uint32")
    return {"global_norm": float(raw[0]), "scale": float(raw[1]), "nonfinite": int(words[2]), "skipped": bool(words[3]),
            "skipped_total": int(words[4]), "norms": raw[8:8 + E].copy(), "scales": raw[8 + E:8 + 2 * E].copy()}


def segment_scale_(flat, plan, scales, skip=None):
    """In place: every element of entry e times scales[e] (one launch over the plan).  skip: a device word; non-zero = write nothing."""
    _f32(flat, "flat")
    _lib.call("skf_segment_scale", _p(flat), _p(plan.dev), plan.n_entries, plan.n_chunks, _p(scales), _p(skip), _stream())
    return flat


def adam_step_clipped(w, g, m, v, state, grad_scale=1.0, scale=None, clipvalue=0.0, skip=None, beta1=0.9, beta2=0.98, eps=1e-9,
                      advance=False):
    """adam_step on gg = (g * grad_scale) * scale[0], clamped to +-clipvalue when clipvalue > 0.  scale: a device float (None = 1);
    skip: two device words {flag, skipped total} such as ``stats[3:5]`` - with the flag set nothing is written, ``iterations`` stays
    and the total goes up; advance: the sweep also closes the step (iterations += 1) unless it is skipped."""
    _lib.call("skf_adam_step_clipped", _p(w), _p(g), _p(m), _p(v), w.numel(), _p(state), float(grad_scale), _p(scale), float(clipvalue),
              _p(skip), beta1, beta2, eps, int(bool(advance)), _stream())


def sgd_momentum_step_clipped(w, g, velocity, state, grad_scale=1.0, scale=None, clipvalue=0.0, skip=None, momentum=0.9, advance=False):
    """sgd_momentum_step with the gradient formed as in ``adam_step_clipped``."""
    _lib.call("skf_sgd_momentum_step_clipped", _p(w), _p(g), _p(velocity), w.numel(), _p(state), float(grad_scale), _p(scale),
              float(clipvalue), _p(skip), momentum, int(bool(advance)), _stream())


def dropout(x, rate, site=0, state=None):
    """Inverted dropout (tf.keras.layers.Dropout in training mode) with the kernels' counter-based mask of (step key, site, element):
    skf_dropout.  rate 0 or no state = the input itself."""
    if rate <= 0.0 or state is None:
        return x
    _f32(x, "x")
    y = torch.empty_like(x)
    _lib.call("skf_dropout", _p(x), _p(y), x.numel(), float(rate), int(site), _p(state), _stream())
    return y


def embed_continuous_fwd(x, W, bias, pos, L=None, rate=0.0, site=0, state=None):
    """Encoder / Decoder embed stage in continuous mode (builders/layers/transformer.py:276,288-296): Dense(5 -> d) of the stroke-5
    rows, * sqrt(d), + pos[:L], dropout.  x (B, ld, 5) float32."""
    _f32(x, "x")
    B, ld = x.shape[0], x.shape[1]
    L = L or ld
    d = W.shape[1]
    out = torch.empty(B, L, d, dtype=torch.float32, device=x.device)
    _lib.call("skf_embed_continuous_fwd", _p(x), ld, B, L, _p(W), _p(bias), d, _p(pos), _p(out), float(rate), int(site), _p(state), _stream())
    return out


def dropout_keep_mask(drop_key, site, rate, n):
    """Host replica of the kernels' counter-based keep mask (for parity tests)."""
    import numpy as np
    out = np.empty(n, dtype=np.uint8)
    _lib.call("skf_dropout_keep_mask", drop_key, site, rate, n, out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)


def sample_uniform(seed, stream_id, step):
    """The uniform of the sampled decode for (seed, stream_id, step): a multiple of 2^-24 in [0, 1) (skf_sample_uniform; host)."""
    return float(_lib.load().skf_sample_uniform(int(seed) & 0xffffffff, int(stream_id) & 0xffffffff, int(step) & 0xffffffff))


def sample_tokens(logits, temperature, top_k, top_p, seed, stream_ids, step):
    """One token per row of logits (B, V) float32, drawn by the selection rule of include/skf.h (skf_decode_sample_tokens: one
    workgroup per row): logits / temperature, top_k largest (0 = off), nucleus top_p (1 = off), inverse CDF in index order with
    u = sample_uniform(seed, stream_ids[b], step).  stream_ids: B integers (sequence or int32 tensor).  -> (B,) int64."""
    _f32(logits, "logits")
    if logits.dim() != 2:
        raise ValueError("logits must be (B, V)")
    _p(logits)                                                   # CPU tensors: SkfError before anything is allocated
    B, V = logits.shape
    dev = logits.device
    step = int(step)
    if step < 0:
        raise ValueError("step must be >= 0")
    if not torch.is_tensor(stream_ids):
        stream_ids = torch.tensor([int(v) for v in stream_ids], dtype=torch.int32)
    stream_ids = stream_ids.to(device=dev, dtype=torch.int32).contiguous()
    if stream_ids.shape != (B,):
        raise ValueError("stream_ids must hold one integer per row")
    smp = _lib.SkfSampling(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed) & 0xffffffff)
    # the launch appends to a running (B, step + 2) token image like the decoder's; only its last column is of interest here
    tokens = torch.zeros(B, step + 2, dtype=torch.int64, device=dev)
    mask = torch.zeros(B, step + 2, dtype=torch.uint8, device=dev)
    flags = torch.zeros(B + 1, dtype=torch.int32, device=dev)                    # eos_seen (B), done_step
    _lib.call("skf_decode_sample_tokens", _p(logits), logits.stride(0), B, V, B, step, -1, _p(tokens), step + 2, _p(mask), step + 2,
              _p(flags), C.c_void_p(flags.data_ptr() + 4 * B), None, None, C.byref(smp), _p(stream_ids), _stream())
    return tokens[:, step + 1].clone()


def beam_step(cand_logp, cand_tok, scores, finished, anc, step, eos, lengths=None):
    """One merge of beam search on caller tensors (skf_beam_advance; the selection rule is in include/skf.h).  n sketches of W beams:
    cand_logp (n W, W) float32 and cand_tok (n W, W) int32: every beam's W candidates; scores (n W,) float32, finished (n W,)
    int32, lengths (n W,) int32 (default zeros): the beams before the step; anc (n W, >= step + 2) int32: the ancestry rows
    of position `step`.  Nothing is modified.  -> dict(parent, token, score, finished, length: (n W,), anc: like anc, row r' =
    the parent's row up to `step`, then r')."""
    _f32(cand_logp, "cand_logp")
    _f32(scores, "scores")
    if cand_logp.dim() != 2 or cand_tok.shape != cand_logp.shape:
        raise ValueError("cand_logp and cand_tok must both be (n * W, W)")
    R, W = cand_logp.shape
    step = int(step)
    if not 1 <= W <= _lib.BEAM_MAX or R % W:
        raise ValueError("need 1 <= W <= %d and n * W rows" % _lib.BEAM_MAX)
    if step < 0 or anc.dim() != 2 or anc.shape[0] != R or anc.shape[1] < step + 2:
        raise ValueError("anc must be (n * W, >= step + 2) and step >= 0")
    _p(cand_logp)
    dev = cand_logp.device
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()      # noqa: E731
    cand_logp, cand_tok = cand_logp.contiguous(), i32(cand_tok)
    sc = scores.to(dev).contiguous().clone()
    fin = i32(finished).clone()
    ln = torch.zeros(R, dtype=torch.int32, device=dev) if lengths is None else i32(lengths).clone()
    if sc.shape != (R,) or fin.shape != (R,) or ln.shape != (R,):
        raise ValueError("scores, finished and lengths hold one entry per beam")
    ld = anc.shape[1]
    tables = torch.zeros(2, R, ld, dtype=torch.int32, device=dev)
    tables[step & 1] = i32(anc)
    tokens = torch.zeros(R, step + 2, dtype=torch.int64, device=dev)
    mask = torch.zeros(R, step + 2, dtype=torch.uint8, device=dev)
    parent = torch.zeros(R, dtype=torch.int32, device=dev)
    _lib.call("skf_beam_advance", _p(cand_logp), _p(cand_tok), R // W, W, step, int(eos), _p(sc), _p(fin), _p(ln), _p(tables), ld,
              _p(tokens), step + 2, _p(mask), step + 2, _p(parent), _stream())
    return dict(parent=parent, token=tokens[:, step + 1].clone(), pad=mask[:, step + 1].clone(), score=sc, finished=fin, length=ln,
                anc=tables[(step + 1) & 1])


def beam_finish(scores, lengths, anc, tokens, beam_width, length_alpha=0.0, ncols=None):
    """The final order of beam search on caller tensors (skf_beam_finish).  scores (n W,) float32, lengths (n W,) int32, anc (n W, ld)
    int32: the ancestry rows, tokens (n W, T) int64: the running image.  -> (tokens (n, W, T) int64: every hypothesis read through
    its ancestry row, zeros from ncols (default T) on; scores (n, W); lengths (n, W)), each sketch ordered by
    score / ((5 + length) / 6)^length_alpha descending, then beam index; the scores are the raw sums."""
    _f32(scores, "scores")
    _p(scores)
    dev = scores.device
    R, W = scores.shape[0], int(beam_width)
    if not 1 <= W <= _lib.BEAM_MAX or R % W or R == 0:
        raise ValueError("need 1 <= W <= %d and n * W rows" % _lib.BEAM_MAX)
    lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
    anc = anc.to(device=dev, dtype=torch.int32).contiguous()
    tokens = tokens.to(device=dev, dtype=torch.int64).contiguous()
    T = tokens.shape[1]
    ncols = T if ncols is None else int(ncols)
    if lengths.shape != (R,) or anc.dim() != 2 or anc.shape[0] != R or tokens.shape[0] != R or not 1 <= ncols <= min(T, anc.shape[1]):
        raise ValueError("lengths (n W,), anc (n W, >= ncols), tokens (n W, T) and 1 <= ncols <= T")
    n = R // W
    out = torch.zeros(n, W, T, dtype=torch.int64, device=dev)
    osc = torch.zeros(n, W, dtype=torch.float32, device=dev)
    oln = torch.zeros(n, W, dtype=torch.int32, device=dev)
    _lib.call("skf_beam_finish", _p(scores.contiguous()), _p(lengths), _p(anc), anc.shape[1], _p(tokens), T, n, W, ncols, T,
              float(length_alpha), _p(out), _p(osc), _p(oln), _stream())
    return out, osc, oln


def row_normalize(x):
    """(N, d) float32 -> rows divided by max(norm, 1e-12), out of place (skf_row_normalize_f32)."""
    _f32(x, "x")
    assert x.dim() == 2
    y = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    _lib.call("skf_row_normalize_f32", _p(x), x.stride(0), x.shape[0], x.shape[1], _p(y), y.stride(0), _stream())
    return y


def knn_topk(queries, gallery, k, exclude=None, metric='l2'):
    """Exact k nearest gallery rows of every query row (skf_knn_topk_f32): queries (Q, d), gallery (G, d) float32 ->
    (indices int32 (Q, k), distances float32 (Q, k)), ascending by squared Euclidean distance, ties to the lower gallery row.
    exclude: int32 (Q,), one gallery row per query left out of its ranking (-1 = none).  metric 'cosine' ranks the row-normalised
    inputs (the distance is then 2 - 2 cos)."""
    if metric not in ('l2', 'cosine'):
        raise ValueError("metric must be 'l2' or 'cosine' (got %r)" % (metric,))
    _f32(queries, "queries"); _f32(gallery, "gallery")
    if queries.dim() != 2 or gallery.dim() != 2 or queries.shape[1] != gallery.shape[1]:
        raise ValueError("queries (Q, d) and gallery (G, d) must share d")
    _p(queries); _p(gallery)                                     # CPU tensors: SkfError before anything is allocated
    if gallery.device != queries.device:
        raise ValueError("queries and gallery must be on one device")
    if exclude is not None:
        if exclude.dtype != torch.int32 or exclude.shape != (queries.shape[0],) or not exclude.is_contiguous():
            raise TypeError("exclude must be a contiguous int32 tensor of shape (Q,)")
    Q, d = queries.shape
    G = gallery.shape[0]
    k = int(k)
    if metric == 'cosine':
        queries, gallery = row_normalize(queries), row_normalize(gallery)
    idx = torch.empty(Q, k, dtype=torch.int32, device=queries.device)
    dist = torch.empty(Q, k, dtype=torch.float32, device=queries.device)
    ws, _ = _workspace_for("skf_knn_workspace_bytes", queries.device, Q, G, k)
    _lib.call("skf_knn_topk_f32", _p(queries), queries.stride(0), Q, _p(gallery), gallery.stride(0), G, d, k, _p(exclude),
              _p(idx), _p(dist), _p(ws), ws.numel(), _stream())
    return idx, dist


INTERP_MODES = {'slerp': 0, 'lerp': 1}


def interpolate(a, b, t, mode='slerp', out=None):
    """T interpolation steps between P pairs of rows (skf_interpolate_f32): a, b (P, d) float32, t a 1-D float32 tensor or a
    sequence of T numbers (taken as float32) -> (P, T, d) float32, [p, j] = the interpolation of (a[p], b[p]) at t[j].
    mode 'slerp': fp64 angle, fp32 weights sin((1 - t) w) / sin w and sin(t w) / sin w; a pair that points the same or the
    opposite way (sin w < 1e-6) returns a[p] in every row.  mode 'lerp': weights 1 - t and t.  t = 0 / t = 1 give a[p] / b[p]
    exactly.  out: a (P, T, d) view to write instead of a new tensor (its rows may sit in a wider buffer; it must not overlap a
    or b)."""
    if mode not in INTERP_MODES:
        raise ValueError("mode must be 'slerp' or 'lerp' (got %r)" % (mode,))
    _f32(a, "a"); _f32(b, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape != b.shape:
        raise ValueError("a and b must both be (P, d) (got %r and %r)" % (tuple(a.shape), tuple(b.shape)))
    _p(a); _p(b)                                                 # CPU tensors: SkfError before anything is allocated
    if b.device != a.device:
        raise ValueError("a and b must be on one device")
    if not torch.is_tensor(t):
        t = torch.tensor([float(v) for v in t], dtype=torch.float32)
    if t.dim() != 1:
        raise ValueError("t must be one-dimensional")
    t = t.to(device=a.device, dtype=torch.float32).contiguous()
    P, d = a.shape
    T = t.shape[0]
    if out is None:
        out = torch.empty(P, T, d, dtype=torch.float32, device=a.device)
    else:
        _f32(out, "out")
        ldo = out.stride(1) if out.dim() == 3 else 0
        if tuple(out.shape) != (P, T, d) or out.device != a.device or out.stride(0) != T * ldo:
            raise ValueError("out must be a (P, T, d) device tensor whose rows p * T + j share one pitch")
    _lib.call("skf_interpolate_f32", _p(a), a.stride(0), _p(b), b.stride(0), P, d, _p(t), T, INTERP_MODES[mode],
              _p(out), out.stride(1), _stream())
    return out


def _kmeans_operands(points, centers):
    _f32(points, "points"); _f32(centers, "centers")
    if points.dim() != 2 or centers.dim() != 2 or points.shape[1] != centers.shape[1]:
        raise ValueError("points (N, d) and centers (K, d) must share d")
    _p(points); _p(centers)                                      # CPU tensors: SkfError before anything is allocated
    if centers.device != points.device:
        raise ValueError("points and centers must be on one device")


def kmeans_assign(points, centers, return_dist=False):
    """Nearest centre of every point (skf_kmeans_assign_f32): points (N, 2), centers (K, 2) float32 -> labels int32 (N,), and
    with return_dist the squared distances float32 (N,).  The distance is fmaf(dy, dy, dx * dx) in fp32; among equal minima the
    lowest centre index wins."""
    _kmeans_operands(points, centers)
    N, d = points.shape
    labels = torch.empty(N, dtype=torch.int32, device=points.device)
    dist = torch.empty(N, dtype=torch.float32, device=points.device) if return_dist else None
    _lib.call("skf_kmeans_assign_f32", _p(points), points.stride(0), N, d, _p(centers), centers.stride(0), centers.shape[0],
              _p(labels), _p(dist), _stream())
    return (labels, dist) if return_dist else labels


def new_kmeans_state(device):
    """Device-resident SkfKmeansState {int32 iterations, converged, n_empty, pad; f64 inertia, shift}, zeroed: one per fit."""
    return torch.zeros(C.sizeof(_lib.SkfKmeansState) // 8, dtype=torch.int64, device=device)


def read_kmeans_state(state):
    """-> dict(iterations, converged, n_empty, inertia, shift) (host sync)."""
    s = _lib.SkfKmeansState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {"iterations": s.iterations, "converged": bool(s.converged), "n_empty": s.n_empty, "inertia": s.inertia, "shift": s.shift}


def kmeans_scale_exp(max_abs):
    """The largest e with max_abs * 2^e < 2^30 (the integer image of a coordinate that skf_kmeans_step_f32 accumulates)."""
    import math
    if not max_abs > 0.0:
        return 0
    return max(-126, min(127, 30 - math.frexp(float(max_abs))[1]))      # max_abs = m * 2^ex, m in [0.5, 1) -> max_abs < 2^ex


def kmeans_step(points, centers, state, scale_exp, tol_abs=-1.0, labels=None, counts=None, workspace=None):
    """One Lloyd iteration (skf_kmeans_step_f32), enqueued on the current stream: labels of `points` against `centers`, then
    `centers` (K, 2) overwritten IN PLACE by the means of their points (a centre without points keeps its coordinates) and `state`
    (new_kmeans_state) updated: iterations += 1, inertia, shift, n_empty, and converged once shift <= tol_abs (tol_abs < 0: never).
    On a converged state the call changes nothing.  scale_exp: kmeans_scale_exp(max |coordinate|), chosen once per fit.
    labels / counts / workspace are allocated when not passed (a fit passes the same ones every iteration).
    -> (labels int32 (N,), counts int32 (K,))."""
    _kmeans_operands(points, centers)
    N, d = points.shape
    K = centers.shape[0]
    dev = points.device
    if state.dtype != torch.int64 or state.numel() * 8 < C.sizeof(_lib.SkfKmeansState) or not state.is_contiguous():
        raise TypeError("state must come from new_kmeans_state")
    labels = torch.empty(N, dtype=torch.int32, device=dev) if labels is None else labels
    counts = torch.empty(K, dtype=torch.int32, device=dev) if counts is None else counts
    if labels.dtype != torch.int32 or labels.shape != (N,) or not labels.is_contiguous():
        raise TypeError("labels must be a contiguous int32 tensor of shape (N,)")
    if counts.dtype != torch.int32 or counts.shape != (K,) or not counts.is_contiguous():
        raise TypeError("counts must be a contiguous int32 tensor of shape (K,)")
    ws = _ws(_lib.load().skf_kmeans_workspace_bytes(N, K), dev) if workspace is None else workspace
    _lib.call("skf_kmeans_step_f32", _p(points), points.stride(0), N, d, _p(centers), centers.stride(0), K, int(scale_exp),
              float(tol_abs), _p(labels), _p(counts), _p(state), _p(ws), ws.numel(), _stream())
    return labels, counts


TSNE_MAX_N = 8192


def _tsne_ws(N, device, workspace):
    if workspace is not None:
        return workspace
    return _ws(_lib.load().skf_tsne_workspace_bytes(N) if 3 <= N <= TSNE_MAX_N else 0, device)


def _tsne_matrix(P, name="P"):
    _f32(P, name)
    if P.dim() != 2 or P.shape[0] != P.shape[1]:
        raise ValueError("%s must be (N, N)" % name)
    _p(P)                                                        # CPU tensors: SkfError before anything is allocated
    return P.shape[0]


def _tsne_points(t, name, N, device):
    _f32(t, name)
    if tuple(t.shape) != (N, 2) or not t.is_contiguous() or t.device != device:
        raise ValueError("%s must be a contiguous (N, 2) float32 tensor on the device of P" % name)
    return t


def tsne_new_affinities(N, device):
    """An (N, N) float32 view whose rows are 16-byte aligned (the row pitch is N rounded up to a multiple of 4)."""
    return torch.empty(N, (N + 3) // 4 * 4, dtype=torch.float32, device=device)[:, :N]


def tsne_affinities(x, perplexity, return_beta=False, out=None, workspace=None):
    """Joint probabilities of exact t-SNE (skf_tsne_affinities_f32): x (N, d) float32 -> P (N, N) float32, symmetric bit for bit,
    zero diagonal, summing to 1; with return_beta also the N precisions (float64) of the rows' Gaussians after the 64-step
    bisection to `perplexity`.  x may be a row view of a wider buffer.  out: an (N, N) view to write instead of a new tensor
    (tsne_new_affinities gives one; its row pitch must be a multiple of 4).  The result is a view with such a pitch."""
    _f32(x, "x")
    if x.dim() != 2:
        raise ValueError("x must be (N, d)")
    _p(x)                                                        # CPU tensors: SkfError before anything is allocated
    N, d = x.shape
    if out is None:
        out = tsne_new_affinities(N if 3 <= N <= TSNE_MAX_N else 4, x.device)    # the library refuses such an N before it looks at P
    else:
        if _tsne_matrix(out, "out") != N or out.device != x.device:
            raise ValueError("out must be an (N, N) float32 tensor on the device of x")
    beta = torch.empty(max(N, 1), dtype=torch.float64, device=x.device) if return_beta else None
    ws = _tsne_ws(N, x.device, workspace)
    _lib.call("skf_tsne_affinities_f32", _p(x), x.stride(0), N, d, float(perplexity), _p(out), out.stride(0), _p(beta),
              _p(ws), ws.numel(), _stream())
    return (out, beta) if return_beta else out


def tsne_step(P, Y, U, gains, exaggeration, momentum, learning_rate, return_grad=False, workspace=None):
    """One gradient-descent iteration of exact t-SNE (skf_tsne_step_f32), enqueued on the current stream, IN PLACE on Y, U
    (velocity) and gains, contiguous (N, 2) float32: the gradient 4 (exaggeration sum_j P_ij q_ij (y_i - y_j) - sum_j q_ij^2
    (y_i - y_j) / Z) from one pass over the pairs, then scikit-learn's gains / momentum update, each operation rounded to float32
    on its own.  P (N, N) float32 may be a row view with a pitch that is a multiple of 4.  return_grad: -> the gradient (N, 2)."""
    N = _tsne_matrix(P)
    for t, name in ((Y, "Y"), (U, "U"), (gains, "gains")):
        _tsne_points(t, name, N, P.device)
    grad = torch.empty(N, 2, dtype=torch.float32, device=P.device) if return_grad else None
    ws = _tsne_ws(N, P.device, workspace)
    _lib.call("skf_tsne_step_f32", _p(P), P.stride(0), N, _p(Y), _p(U), _p(gains), _p(grad), float(exaggeration), float(momentum),
              float(learning_rate), _p(ws), ws.numel(), _stream())
    return grad


def tsne_kl(P, Y, workspace=None):
    """KL(P || Q) of the embedding Y (skf_tsne_kl_f32): P (N, N), Y (N, 2) float32 -> a float64 tensor of one element on the
    device (no host sync), the sum over P_ij > 0 of P_ij log(P_ij / Q_ij), accumulated in float64."""
    N = _tsne_matrix(P)
    _tsne_points(Y, "Y", N, P.device)
    out = torch.empty(1, dtype=torch.float64, device=P.device)
    ws = _tsne_ws(N, P.device, workspace)
    _lib.call("skf_tsne_kl_f32", _p(P), P.stride(0), N, _p(Y), _p(out), _p(ws), ws.numel(), _stream())
    return out


SKETCH_KINDS = {'stroke3': 0, 'stroke5': 1, 'dict_tokens': 2, 'grid_tokens': 3}       # SKF_SKETCH_* of include/skf.h


def sketch_points(data, kind, lengths=None, centers=None, resolution=None, T=None):
    """Any sketch encoding -> drawable points (skf_sketch_points).  kind 'stroke3': data (B, T, 3) float32 offsets + lengths
    int32 (B,); 'stroke5': data (B, T, 5) float32; 'dict_tokens': data (B, ld) int64 ids + centers (K, 2) float32;
    'grid_tokens': data (B, ld) int64 ids + the grid resolution.  T: positions read per sketch (tokens only; default ld).
    Returns (xy (B, T, 2) float32 absolute positions, pen (B, T) uint8, n_points (B,) int32, bounds (B, 4) float32 =
    (min x, min y, max x, max y)); rows behind n_points are zero.  An empty sketch has n_points = 0; an id outside the vocabulary
    is skipped."""
    if kind not in SKETCH_KINDS:
        raise ValueError("kind must be one of %s (got %r)" % (sorted(SKETCH_KINDS), kind))
    _p(data)                                                     # CPU tensors: SkfError before anything is allocated
    K = 0
    if kind in ('stroke3', 'stroke5'):
        width = 3 if kind == 'stroke3' else 5
        if data.dtype != torch.float32 or data.dim() != 3 or data.shape[2] != width or not data.is_contiguous():
            raise TypeError("%s data must be a contiguous float32 tensor of shape (B, T, %d)" % (kind, width))
        B, ld = data.shape[0], data.shape[1] * width
        if T is not None and int(T) != data.shape[1]:
            raise ValueError("T of stroke data is its second dimension")
        T = data.shape[1]
        if kind == 'stroke3':
            if lengths is None or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous() \
                    or lengths.device != data.device:
                raise TypeError("stroke3 needs lengths: a contiguous int32 tensor of shape (B,) on the device of data")
        else:
            lengths = None
        centers = None
    else:
        if data.dtype != torch.int64 or data.dim() != 2 or data.stride(1) != 1:
            raise TypeError("token data must be an int64 tensor of shape (B, ld) with a unit innermost stride")
        B, ld = data.shape[0], data.stride(0)
        T = data.shape[1] if T is None else int(T)
        if T < 1 or T > data.shape[1]:
            raise ValueError("T must be in [1, %d]" % data.shape[1])
        lengths = None
        if kind == 'dict_tokens':
            if centers is None or centers.dtype != torch.float32 or centers.dim() != 2 or centers.shape[1] != 2 \
                    or not centers.is_contiguous() or centers.device != data.device:
                raise TypeError("dict_tokens needs centers: a contiguous float32 tensor of shape (K, 2) on the device of data")
            K = centers.shape[0]
        else:
            if resolution is None:
                raise ValueError("grid_tokens needs the grid resolution")
            K, centers = int(resolution), None
    if B < 1 or T < 1:
        raise ValueError("sketch_points needs at least one sketch and one position")
    dev = data.device
    xy = torch.empty(B, T, 2, dtype=torch.float32, device=dev)
    pen = torch.empty(B, T, dtype=torch.uint8, device=dev)
    n = torch.empty(B, dtype=torch.int32, device=dev)
    bounds = torch.empty(B, 4, dtype=torch.float32, device=dev)
    _lib.call("skf_sketch_points", SKETCH_KINDS[kind], _p(data), ld, _p(lengths), _p(centers), K, B, T, _p(xy), _p(pen), _p(n),
              _p(bounds), _stream())
    return xy, pen, n, bounds


def rasterize(xy, pen, n_points, frames, size, line_width=1.5, margin=2.0, out=None):
    """Points -> anti-aliased coverage images (skf_rasterize_f32): xy (B, T, 2) float32, pen (B, T) uint8, n_points (B,) int32 as
    sketch_points returns them, frames (B, 4) float32 = the box (x0, y0, x1, y1) every sketch is fitted into, size = (H, W) ->
    (B, H, W) float32, ink 1, paper 0: coverage = clamp(0.5 + line_width / 2 - distance to the nearest stroke, 0, 1) at every
    pixel centre.  include/skf.h has the frame rule."""
    H, W = (int(v) for v in size)
    _p(xy)
    if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[2] != 2 or not xy.is_contiguous():
        raise TypeError("xy must be a contiguous float32 tensor of shape (B, T, 2)")
    B, T = xy.shape[0], xy.shape[1]
    dev = xy.device
    if pen.dtype != torch.uint8 or tuple(pen.shape) != (B, T) or not pen.is_contiguous() or pen.device != dev:
        raise TypeError("pen must be a contiguous uint8 tensor of shape (B, T) on the device of xy")
    if n_points.dtype != torch.int32 or tuple(n_points.shape) != (B,) or not n_points.is_contiguous() or n_points.device != dev:
        raise TypeError("n_points must be a contiguous int32 tensor of shape (B,) on the device of xy")
    if frames.dtype != torch.float32 or tuple(frames.shape) != (B, 4) or not frames.is_contiguous() or frames.device != dev:
        raise TypeError("frames must be a contiguous float32 tensor of shape (B, 4) on the device of xy")
    if out is None:
        out = torch.empty(B, max(H, 0), max(W, 0), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, H, W) or not out.is_contiguous() or out.device != dev:
        raise TypeError("out must be a contiguous float32 tensor of shape (B, H, W) on the device of xy")
    _lib.call("skf_rasterize_f32", _p(xy), _p(pen), _p(n_points), _p(frames), B, T, H, W, float(line_width), float(margin), _p(out),
              _stream())
    return out


def raster_overlap(a, b):
    """(sum min(a, b), sum max(a, b)) of every pair of images (skf_raster_overlap_f32): a, b (B, ...) float32 of one shape ->
    (B, 2) float32, summed in a fixed order (bit-reproducible; an image with itself gives two equal sums)."""
    _f32(a, "a"); _f32(b, "b")
    _p(a); _p(b)
    if a.dim() < 2 or a.shape != b.shape or a.device != b.device:
        raise ValueError("a and b must be two (B, ...) tensors of one shape on one device")
    B = a.shape[0]
    a2, b2 = a.reshape(B, -1), b.reshape(B, -1)
    if a2.stride(1) != 1 or b2.stride(1) != 1:
        raise ValueError("the images of a and b must be contiguous")
    out = torch.empty(B, 2, dtype=torch.float32, device=a.device)
    _lib.call("skf_raster_overlap_f32", _p(a2), a2.stride(0), _p(b2), b2.stride(0), B, a2.shape[1], _p(out), _stream())
    return out


def nearest_center(points, centers):
    """Nearest dictionary centre of every point by the tokenizer's float64 rule (skf_nearest_center_f64): points (P, 2) float32,
    centers (K, 2) float64 -> labels int32 (P,).  d = (x - cx)^2 + (y - cy)^2 with every operation rounded to float64 on its own
    (no fused multiply-add); among equal minima the lowest index wins - Tokenizer.nearest_center's numpy path, bit for bit."""
    _p(points); _p(centers)                                      # CPU tensors: SkfError before anything is allocated
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2 or points.stride(1) != 1:
        raise TypeError("points must be a float32 tensor of shape (P, 2) with a unit innermost stride")
    P, K = points.shape[0], _centers(centers)
    if centers.device != points.device:
        raise ValueError("points and centers must be on one device")
    if P < 1 or not 1 <= K <= 4096:
        raise ValueError("nearest_center needs at least one point and 1 <= K <= 4096 centres")
    labels = torch.empty(P, dtype=torch.int32, device=points.device)
    _lib.call("skf_nearest_center_f64", _p(points), points.stride(0), P, _p(centers), K, _p(labels), _stream())
    return labels


ENCODE_MODES = {'dict': 0, 'grid': 1, 'stroke5': 2}               # SKF_ENCODE_* of include/skf.h


def sketch_encode(flat, offsets, mode, max_seq_len, centers=None, resolution=None, clamp=True, return_scale=False):
    """Raw stroke-3 sketches -> model input (skf_sketch_encode), bit-equal to the loader's per-sketch host pipeline.  flat (P, 3)
    float32 rows (dx, dy, pen) of N sketches back to back, offsets (N + 1) int64 on the same device, non-decreasing from 0 to P
    (the caller builds them on the host and checks that there: preprocess.pack_ragged).  mode 'dict': centers (K, 2) float64 ->
    (N, L) int64; 'grid': the even resolution -> (N, L) int64; 'stroke5' -> (N, L, 5) float32.  clamp: all three columns to +-1000
    first.  With return_scale also the divisor of every sketch, float32 (N,).  include/skf.h has the definition."""
    if mode not in ENCODE_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (sorted(ENCODE_MODES), mode))
    (P, N), L, K = _ragged(flat, offsets, "sketch_encode", limit=False), int(max_seq_len), 0
    if L < 2:
        raise ValueError("max_seq_len must be at least 2")
    if mode == 'dict':
        if centers is None:
            raise ValueError("mode 'dict' needs centers")
        K = _centers(centers, beside=(flat, "flat"))
        if not 1 <= K <= 4096:
            raise ValueError("the dictionary must hold 1 <= K <= 4096 centres")
    else:
        centers = None
        if mode == 'grid':
            if resolution is None:
                raise ValueError("mode 'grid' needs the grid resolution")
            K = int(resolution)
            if K < 2 or K > 32768 or K % 2:
                raise ValueError("the grid resolution must be even, in [2, 32768]")
    dev = flat.device
    out = torch.empty((N, L, 5) if mode == 'stroke5' else (N, L), dtype=torch.float32 if mode == 'stroke5' else torch.int64, device=dev)
    scale = torch.empty(N, dtype=torch.float32, device=dev) if return_scale else None
    ws, nbytes = _workspace_for("skf_sketch_encode_workspace_bytes", dev, P, N)
    _lib.call("skf_sketch_encode", _p(flat), P, _p(offsets), N, ENCODE_MODES[mode], _p(centers), K, L, 1 if clamp else 0, _p(out),
              _p(scale), _p(ws), nbytes, _stream())
    return (out, scale) if return_scale else out


def sketch_augment(flat, offsets, rnd, scale_factor, prob, clamp=True):
    """The training augmentation of continuous sketches (skf_sketch_augment): random scale, then point dropout, bit-equal to the
    loader's host `_augment_sketch` under the same draws.  flat (P, 3) float32 and offsets (N + 1) int64 as for sketch_encode; rnd
    (2 N + P) float64 on the same device, in the order the host draws: per sketch ux, uy, then one draw per point
    (np.random.random(size=2 * N + P) is that stream).  0 <= scale_factor < 1, 0 < prob <= 1.  clamp: all three columns to +-1000
    first.  -> (out_flat (P', 3) float32, out_offsets (N + 1) int64): the augmented sketches back to back, ready for sketch_encode
    with clamp=False.  Reading P' = out_offsets[N] is one small device-to-host copy that waits for the current stream: sketch_encode
    needs offsets that cover its flat exactly, so the rows come back sliced to P' and never at their capacity P."""
    _p(rnd)                                                      # CPU tensors: SkfError before anything is allocated
    P, N = _ragged(flat, offsets, "sketch_augment")
    if rnd.dtype != torch.float64 or rnd.dim() != 1 or not rnd.is_contiguous() or rnd.device != flat.device:
        raise TypeError("rnd must be a contiguous float64 tensor of shape (2 N + P,) on the device of flat")
    if rnd.shape[0] != 2 * N + P:
        raise ValueError("rnd must hold 2 N + P = %d draws (got %d)" % (2 * N + P, rnd.shape[0]))
    scale_factor, prob = float(scale_factor), float(prob)
    if not 0.0 <= scale_factor < 1.0:
        raise ValueError("scale_factor must be in [0, 1)")
    if not 0.0 < prob <= 1.0:
        raise ValueError("prob must be in (0, 1]")
    dev = flat.device
    out_flat = torch.empty(P, 3, dtype=torch.float32, device=dev)
    out_offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace_for("skf_sketch_augment_workspace_bytes", dev, P, N)
    _lib.call("skf_sketch_augment", _p(flat), P, _p(offsets), N, _p(rnd), scale_factor, prob, 1 if clamp else 0, _p(out_flat),
              _p(out_offsets), _p(ws), nbytes, _stream())
    return _compacted(out_flat, out_offsets)


RDP_LDS_POINTS = 512                                             # SKF_RDP_LDS_POINTS of include/skf.h


def _rdp_epsilon(epsilon):
    epsilon = float(epsilon)
    if not 0.0 <= epsilon < float("inf"):                        # (false for a NaN)
        raise ValueError("epsilon must be finite and not negative (got %r)" % epsilon)
    return epsilon


def rdp_keep(xy, stroke_offsets, epsilon):
    """Ramer-Douglas-Peucker keep mask of S polylines (skf_rdp_f32), bit-equal to the host restatement of the rule in
    include/skf.h.  xy (P, 2) float32 absolute points with a unit innermost stride (the row stride is free); stroke_offsets (S + 1)
    int64 on the same device, non-decreasing from 0 to P (the caller checks that on the host); epsilon finite, >= 0, in the units
    of xy.  -> uint8 (P,): 1 = kept.  The ends of every polyline are kept; a polyline of any length is accepted."""
    _p(xy); _p(stroke_offsets)                                   # CPU tensors: SkfError before anything is allocated
    if xy.dtype != torch.float32 or xy.dim() != 2 or xy.shape[1] != 2 or xy.stride(1) != 1:
        raise TypeError("xy must be a float32 tensor of shape (P, 2) with a unit innermost stride")
    P, S = _ragged_offsets(stroke_offsets, xy, "rdp_keep", names=("stroke_offsets", "S", "xy", "polyline"))
    epsilon = _rdp_epsilon(epsilon)
    ldp = xy.stride(0) if P > 1 else 2                           # (the row stride of a single row is never used)
    if ldp < 2:                                                  # an expanded or overlapping view: rows the tensor does not own
        raise ValueError("the rows of xy must not overlap (row stride %d < 2)" % ldp)
    if ldp >= 1 << 31:
        raise ValueError("the row stride of xy must be below 2^31")
    keep = torch.empty(P, dtype=torch.uint8, device=xy.device)
    ws, nbytes = _workspace_for("skf_rdp_workspace_bytes", xy.device, P)
    _lib.call("skf_rdp_f32", _p(xy), ldp, P, _p(stroke_offsets), S, epsilon, _p(keep), _p(ws), nbytes, _stream())
    return keep


def stroke3_simplify(flat, offsets, epsilon):
    """Stroke-3 sketches simplified stroke by stroke (skf_stroke3_simplify): positions by the sequential fp32 running sum, the RDP
    rule of include/skf.h per stroke, the kept rows as offsets from the kept row before them.  flat (P, 3) float32 and offsets
    (N + 1) int64 as for sketch_encode.  -> (out_flat (P', 3) float32, out_offsets (N + 1) int64).  Stroke ends are always kept:
    pen values and the number of strokes do not change.  Reading P' = out_offsets[N] is one small device-to-host copy that waits
    for the current stream."""
    P, N = _ragged(flat, offsets, "stroke3_simplify")
    epsilon = _rdp_epsilon(epsilon)
    dev = flat.device
    out_flat = torch.empty(P, 3, dtype=torch.float32, device=dev)
    out_offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace_for("skf_stroke3_simplify_workspace_bytes", dev, P, N)
    _lib.call("skf_stroke3_simplify", _p(flat), P, _p(offsets), N, epsilon, 0, _p(out_flat), _p(out_offsets), _p(ws), nbytes, _stream())
    return _compacted(out_flat, out_offsets)


RESAMPLE_MAX_N = 65536                                           # SKF_RESAMPLE_MAX_N of include/skf.h
RESAMPLE_MAX_COORD = 16384                                       # SKF_RESAMPLE_MAX_COORD: beyond it the arc length may overflow int64


def _resample_args(xy, stroke_offsets, who):
    """The checks the resampling entry points share -> (P, S, ldp)"""
    _p(xy); _p(stroke_offsets)                                   # CPU tensors: SkfError before anything is allocated
    if xy.dtype != torch.float32 or xy.dim() != 2 or xy.shape[1] != 2 or xy.stride(1) != 1:
        raise TypeError("xy must be a float32 tensor of shape (P, 2) with a unit innermost stride")
    P, S = _ragged_offsets(stroke_offsets, xy, who, names=("stroke_offsets", "S", "xy", "polyline"))
    ldp = xy.stride(0) if P > 1 else 2                           # (the row stride of a single row is never used)
    if ldp < 2:                                                  # an expanded or overlapping view: rows the tensor does not own
        raise ValueError("the rows of xy must not overlap (row stride %d < 2)" % ldp)
    if ldp >= 1 << 31:
        raise ValueError("the row stride of xy must be below 2^31")
    return P, S, ldp


def _resample_spacing(spacing):
    spacing = float(spacing)
    if not (spacing < 7e13 and spacing * 65536.0 > 0.5):         # (false for a NaN); rint(0.5) is 0
        raise ValueError("spacing must be finite, below 7e13, with rint(spacing * 2^16) >= 1 (got %r)" % spacing)
    return spacing


def polyline_resample_offsets(xy, stroke_offsets, spacing, return_workspace=False):
    """The count phase of polyline_resample alone (skf_polyline_resample_count): -> out_offsets (S + 1) int64 on the device, the
    offsets of the resampled polylines, out_offsets[S] = the number of rows polyline_resample would return.  Nothing is read back.
    return_workspace: also (workspace, its size), holding the arc-length tables the emit phase reads."""
    P, S, ldp = _resample_args(xy, stroke_offsets, "polyline_resample")
    spacing = _resample_spacing(spacing)
    out_offsets = torch.empty(S + 1, dtype=torch.int64, device=xy.device)
    ws, nbytes = _workspace_for("skf_polyline_resample_workspace_bytes", xy.device, P, S)
    _lib.call("skf_polyline_resample_count", _p(xy), ldp, P, _p(stroke_offsets), S, spacing, _p(out_offsets), _p(ws), nbytes, _stream())
    return (out_offsets, ws, nbytes) if return_workspace else out_offsets


def polyline_resample(xy, stroke_offsets, spacing):
    """S polylines resampled along their arc length at `spacing` (skf_polyline_resample_count / _emit), bit-equal to the host
    restatement of the rule in include/skf.h.  xy (P, 2) float32 absolute points with a unit innermost stride (the row stride is
    free), |x|, |y| <= 2^14 and finite (the caller's contract: nothing is read back to check it; simplify.resample_lines checks on
    the host); stroke_offsets (S + 1) int64 on the same device, non-decreasing from 0 to P.  -> (out_xy (P', 2) float32, out_offsets
    (S + 1) int64): a polyline of arc length L gives ceil(L / spacing) + 1 rows, its ends bit for bit; an empty one gives none.
    Two phases with one 8-byte read-back of P' = out_offsets[S] between them, which waits for the current stream: the rows cannot be
    allocated before their number is known."""
    P, S, ldp = _resample_args(xy, stroke_offsets, "polyline_resample")
    out_offsets, ws, nbytes = polyline_resample_offsets(xy, stroke_offsets, spacing, return_workspace=True)
    rows = int(out_offsets[-1].item())
    if rows >= (1 << 31) - 1:
        raise ValueError("polyline_resample: the result needs 2^31 rows or more; cut the batch or use a larger spacing")
    out_xy = torch.empty(rows, 2, dtype=torch.float32, device=xy.device)
    if rows:
        _lib.call("skf_polyline_resample_emit", _p(xy), ldp, P, _p(stroke_offsets), S, float(spacing), _p(out_offsets), _p(out_xy), rows,
                  _p(ws), nbytes, _stream())
    return out_xy, out_offsets


def polyline_resample_n(xy, stroke_offsets, n_out):
    """S polylines resampled to n_out points each, equally spaced along the arc length (skf_polyline_resample_n), bit-equal to the
    host restatement.  Arguments as for polyline_resample; 2 <= n_out <= 65536.  -> (S, n_out, 2) float32: the ends bit for bit, a
    polyline of arc length 0 as n_out copies of its first point, an empty one as n_out rows (0, 0).  No read-back."""
    P, S, ldp = _resample_args(xy, stroke_offsets, "polyline_resample_n")
    n_out = int(n_out)
    if not 2 <= n_out <= RESAMPLE_MAX_N:
        raise ValueError("n_out must be in [2, %d] (got %d)" % (RESAMPLE_MAX_N, n_out))
    out = torch.empty(S, n_out, 2, dtype=torch.float32, device=xy.device)
    ws, nbytes = _workspace_for("skf_polyline_resample_workspace_bytes", xy.device, P, S)
    _lib.call("skf_polyline_resample_n", _p(xy), ldp, P, _p(stroke_offsets), S, n_out, _p(out), _p(ws), nbytes, _stream())
    return out


FLATTEN_MAX_N = 4096                                             # SKF_FLATTEN_MAX_N of include/skf.h


def _flatten_args(ctrl, kind, path_offsets, who):
    """The checks the flattening entry points share -> (G, S)"""
    _p(ctrl); _p(kind); _p(path_offsets)                         # CPU tensors: SkfError before anything is allocated
    if ctrl.dtype != torch.float64 or ctrl.dim() != 3 or tuple(ctrl.shape[1:]) != (4, 2) or not ctrl.is_contiguous():
        raise TypeError("ctrl must be a contiguous float64 tensor of shape (G, 4, 2)")
    if kind.dtype != torch.int32 or kind.dim() != 1 or kind.shape[0] != ctrl.shape[0] or not kind.is_contiguous() \
            or kind.device != ctrl.device:
        raise TypeError("kind must be a contiguous int32 tensor of shape (G,) on the device of ctrl")
    return _ragged_offsets(path_offsets, ctrl, who, names=("path_offsets", "S", "ctrl", "subpath"))


def _flatten_tol(tol):
    tol = float(tol)
    if not 0.0 < tol < float("inf"):                             # (false for a NaN)
        raise ValueError("tol must be finite and above 0 (got %r)" % tol)
    return tol


def path_flatten_offsets(ctrl, kind, path_offsets, tol, return_workspace=False):
    """The count phase of path_flatten alone (skf_path_flatten_count): -> out_offsets (S + 1) int64 on the device, the offsets of
    the flattened subpaths, out_offsets[S] = the number of rows path_flatten would return.  Nothing is read back.
    return_workspace: also (workspace, its size), holding the running piece counts the emit phase reads."""
    G, S = _flatten_args(ctrl, kind, path_offsets, "path_flatten")
    tol = _flatten_tol(tol)
    out_offsets = torch.empty(S + 1, dtype=torch.int64, device=ctrl.device)
    ws, nbytes = _workspace_for("skf_path_flatten_workspace_bytes", ctrl.device, G, S)
    _lib.call("skf_path_flatten_count", _p(ctrl), _p(kind), G, _p(path_offsets), S, tol, _p(out_offsets), _p(ws), nbytes, _stream())
    return (out_offsets, ws, nbytes) if return_workspace else out_offsets


def path_flatten(ctrl, kind, path_offsets, tol):
    """S subpaths of lines and cubic Bezier segments flattened to polylines that stay within `tol` of the curves
    (skf_path_flatten_count / _emit), bit-equal to the host restatement of the rule in include/skf.h.  ctrl (G, 4, 2) float64
    control points p0 .. p3, absolute; kind (G,) int32, 1 = cubic, anything else a line from p0 to p3; path_offsets (S + 1) int64
    on the same device, non-decreasing from 0 to G; tol finite, > 0, in the units of ctrl.  -> (out_xy (P', 2) float32, out_offsets
    (S + 1) int64): a subpath gives 1 + the sum of its segments' piece counts rows, the segment ends bit for bit; an empty one
    gives none.  The pair is a valid (xy, stroke_offsets) for rdp_keep, polyline_resample and polyline_resample_n.  Two phases with
    one 8-byte read-back of P' = out_offsets[S] between them, which waits for the current stream: the rows cannot be allocated
    before their number is known."""
    G, S = _flatten_args(ctrl, kind, path_offsets, "path_flatten")
    out_offsets, ws, nbytes = path_flatten_offsets(ctrl, kind, path_offsets, tol, return_workspace=True)
    rows = int(out_offsets[-1].item())
    if rows >= (1 << 31) - 1:
        raise ValueError("path_flatten: the result needs 2^31 rows or more; cut the batch or use a larger tol")
    out_xy = torch.empty(rows, 2, dtype=torch.float32, device=ctrl.device)
    if rows:
        _lib.call("skf_path_flatten_emit", _p(ctrl), _p(kind), G, _p(path_offsets), S, float(tol), _p(out_offsets), _p(out_xy), rows,
                  _p(ws), nbytes, _stream())
    return out_xy, out_offsets


def stroke_table(flat, offsets):
    """The strokes of a ragged batch of stroke-3 sketches (skf_stroke_table; the rule is in include/skf.h).  flat (P, 3) float32
    and offsets (N + 1) int64 as for sketch_encode.  -> (sketch_strokes (N + 1) int64: sketch s owns the global strokes
    sketch_strokes[s] .. sketch_strokes[s + 1] - 1; stroke_rows (T + 1) int64: the first flat row of every stroke, then P;
    stroke_ends (T, 4) float32: the absolute position of the stroke's first and last row).  Reading T = sketch_strokes[N] is one
    8-byte device-to-host copy that waits for the current stream."""
    P, N = _ragged(flat, offsets, "stroke_table")
    dev = flat.device
    sketch_strokes = torch.empty(N + 1, dtype=torch.int64, device=dev)
    stroke_rows = torch.empty(P + 1, dtype=torch.int64, device=dev)
    stroke_ends = torch.empty(P, 4, dtype=torch.float32, device=dev)
    ws, nbytes = _workspace_for("skf_stroke_table_workspace_bytes", dev, P, N)
    _lib.call("skf_stroke_table", _p(flat), P, _p(offsets), N, 0, _p(sketch_strokes), _p(stroke_rows), _p(stroke_ends), _p(ws), nbytes,
              _stream())
    T = min(int(sketch_strokes[-1].item()), P)
    return sketch_strokes, stroke_rows[:T + 1], stroke_ends[:T]


def _stroke_edit_args(flat, offsets, src, sel_offsets, sel, table):
    """The checks of stroke_edit -> (P, N, M, Q, T, table)"""
    P, N = _ragged(flat, offsets, "stroke_edit")
    dev = flat.device
    for t, name, dtype in ((src, "src", torch.int32), (sel_offsets, "sel_offsets", torch.int64), (sel, "sel", torch.int32)):
        _p(t)                                                    # CPU tensors: SkfError before anything is allocated
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
            raise TypeError("%s must be a contiguous %s vector on the device of flat" % (name, str(dtype).replace("torch.", "")))
    M, Q = src.shape[0], sel.shape[0]
    if M < 1:
        raise ValueError("stroke_edit needs at least one output sketch")
    if sel_offsets.shape[0] != M + 1:
        raise ValueError("sel_offsets must hold M + 1 = %d entries (got %d)" % (M + 1, sel_offsets.shape[0]))
    if Q >= 1 << 31:
        raise ValueError("stroke_edit takes fewer than 2^31 selected strokes")
    if table is None:
        table = stroke_table(flat, offsets)
    sketch_strokes, stroke_rows, stroke_ends = table
    T = stroke_rows.shape[0] - 1
    for t, name, dtype, shape in ((sketch_strokes, "sketch_strokes", torch.int64, (N + 1,)), (stroke_rows, "stroke_rows", torch.int64, (T + 1,)),
                                  (stroke_ends, "stroke_ends", torch.float32, (T, 4))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise TypeError("table: %s must be a contiguous %s tensor of shape %r on the device of flat, as stroke_table returns it"
                            % (name, str(dtype).replace("torch.", ""), shape))
    if T < 0 or T > P:
        raise ValueError("table: stroke_rows must hold between 1 and P + 1 entries")
    return P, N, M, Q, T, table


def stroke_edit(flat, offsets, src, sel_offsets, sel, table=None):
    """New sketches out of the strokes of old ones (skf_stroke_edit_count / _emit; the rule is in include/skf.h), bit-equal to the
    host restatement.  flat (P, 3) float32 and offsets (N + 1) int64 as for sketch_encode; src (M,) int32: the source sketch of
    every output sketch; sel_offsets (M + 1) int64, non-decreasing from 0 to Q; sel (Q,) int32: k >= 0 = stroke k of the source
    as stored, ~k = the same stroke drawn backwards; an entry that names no stroke gives no rows.  table: what stroke_table(flat,
    offsets) returned, to edit one batch several times.  -> (out_flat (P', 3) float32, out_offsets (M + 1) int64), (0, 3) when
    nothing is selected.  Two phases with one 8-byte read-back of P' = out_offsets[M] between them, which waits for the current
    stream (and one more inside stroke_table when no table is given).  sel_offsets that do not run from 0 to Q without
    decreasing are refused (ValueError): the check runs on the device and travels with that read-back."""
    P, N, M, Q, T, (sketch_strokes, stroke_rows, stroke_ends) = _stroke_edit_args(flat, offsets, src, sel_offsets, sel, table)
    dev = flat.device
    out_offsets = torch.empty(M + 1, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace_for("skf_stroke_edit_workspace_bytes", dev, P, N, M, Q)
    _lib.call("skf_stroke_edit_count", P, _p(sketch_strokes), N, _p(stroke_rows), T, _p(src), _p(sel_offsets), M, _p(sel) if Q else None, Q,
              0, _p(out_offsets), _p(ws), nbytes, _stream())
    # the lists must run from 0 to Q without decreasing (overlapping lists would give an entry two writers); checked on the device
    # and read back with the row count: -1 in its place
    ordered = (sel_offsets[1:] >= sel_offsets[:-1]).all() & (sel_offsets[0] == 0) & (sel_offsets[-1] == Q)
    rows = int(torch.where(ordered, out_offsets[-1], -1).item())
    if rows < 0:
        raise ValueError("sel_offsets must run from 0 to the number of selected strokes (%d) without decreasing" % Q)
    if rows >= (1 << 31) - 1:
        raise ValueError("stroke_edit: the result needs 2^31 rows or more; cut the edit into several calls")
    out_flat = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    if rows:
        _lib.call("skf_stroke_edit_emit", _p(flat), P, _p(sketch_strokes), N, _p(stroke_rows), _p(stroke_ends), T, _p(src), _p(sel_offsets),
                  M, _p(sel), Q, 0, _p(out_offsets), _p(out_flat), rows, _p(ws), nbytes, _stream())
    return out_flat, out_offsets


ALIGN_MAX_LEN = 512                                              # SKF_ALIGN_MAX_LEN of include/skf.h


def _align_lengths(t, name, N, dev):
    if t.dtype != torch.int32 or tuple(t.shape) != (N,) or not t.is_contiguous() or t.device != dev:
        raise TypeError("%s must be a contiguous int32 tensor of shape (%d,) on the device of its rows" % (name, N))
    return t


def _align_check(Na, Nb, Ta, Tb, cross):
    if Na < 1 or Nb < 1 or Ta < 1 or Tb < 1:
        raise ValueError("both sides need at least one row and one position")
    if Ta > ALIGN_MAX_LEN or Tb > ALIGN_MAX_LEN:
        raise ValueError("rows hold at most %d positions (got %d and %d)" % (ALIGN_MAX_LEN, Ta, Tb))
    if not cross and Na != Nb:
        raise ValueError("paired mode needs as many rows of a as of b (got %d and %d); cross=True compares every pair" % (Na, Nb))


def edit_distance(a, b, len_a, len_b, cross=False):
    """Unit-cost Levenshtein distance between rows of token ids (skf_edit_distance_i64): a (Na, Ta), b (Nb, Tb) int64 with a unit
    innermost stride (the row stride is free: a view into a wider row is fine), len_a (Na,), len_b (Nb,) int32 = how many ids of
    each row count (clamped to [0, T] on the device), T <= 512.  -> int32 (Na,) pairing row i with row i, or with cross=True
    (Na, Nb) holding every pair.  Exact; ids are compared as 64-bit integers; an empty side gives the other side's length."""
    for t, name in ((a, "a"), (b, "b")):
        if t.dtype != torch.int64 or t.dim() != 2:
            raise TypeError("%s must be an int64 tensor of shape (N, T)" % name)
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError("%s must have a unit innermost stride and rows that do not overlap" % name)
    if b.device != a.device:
        raise ValueError("a and b must be on one device")
    (Na, Ta), (Nb, Tb) = a.shape, b.shape
    _align_lengths(len_a, "len_a", Na, a.device); _align_lengths(len_b, "len_b", Nb, a.device)
    _align_check(Na, Nb, Ta, Tb, cross)
    _p(a); _p(b); _p(len_a); _p(len_b)                           # CPU tensors: SkfError before anything is allocated
    out = torch.empty((Na, Nb) if cross else (Na,), dtype=torch.int32, device=a.device)
    _lib.call("skf_edit_distance_i64", _p(a), max(a.stride(0), Ta), _p(len_a), Na, Ta, _p(b), max(b.stride(0), Tb), _p(len_b), Nb, Tb,
              1 if cross else 0, _p(out), _stream())
    return out


def dtw_distance(xy_a, n_a, xy_b, n_b, cross=False):
    """Dynamic time warping between point rows (skf_dtw_f32): xy_a (Na, Ta, 2), xy_b (Nb, Tb, 2) float32 absolute positions as
    sketch_points returns them (points contiguous; the row stride is free), n_a (Na,), n_b (Nb,) int32 = the points of each row
    (clamped to [0, T] on the device), T <= 512.  -> float32 (Na,), or with cross=True (Na, Nb): the accumulated Euclidean
    distance along the best monotone alignment, not normalised.  An empty row stands for the single point (0, 0).  Every cell is
    c + min(up, left, diagonal) in float32 without a fused multiply-add: bit-equal to a float32 numpy restatement."""
    for t, name in ((xy_a, "xy_a"), (xy_b, "xy_b")):
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 2:
            raise TypeError("%s must be a float32 tensor of shape (N, T, 2)" % name)
        if t.stride(2) != 1 or (t.shape[1] > 1 and t.stride(1) != 2) or (t.shape[0] > 1 and t.stride(0) < 2 * t.shape[1]):
            raise ValueError("%s must hold contiguous (x, y) points in rows that do not overlap" % name)
    if xy_b.device != xy_a.device:
        raise ValueError("xy_a and xy_b must be on one device")
    (Na, Ta), (Nb, Tb) = xy_a.shape[:2], xy_b.shape[:2]
    _align_lengths(n_a, "n_a", Na, xy_a.device); _align_lengths(n_b, "n_b", Nb, xy_a.device)
    _align_check(Na, Nb, Ta, Tb, cross)
    _p(xy_a); _p(xy_b); _p(n_a); _p(n_b)                         # CPU tensors: SkfError before anything is allocated
    out = torch.empty((Na, Nb) if cross else (Na,), dtype=torch.float32, device=xy_a.device)
    _lib.call("skf_dtw_f32", _p(xy_a), max(xy_a.stride(0), 2 * Ta), _p(n_a), Na, Ta, _p(xy_b), max(xy_b.stride(0), 2 * Tb), _p(n_b), Nb, Tb,
              1 if cross else 0, _p(out), _stream())
    return out


SHAPE_GALLERY_BLOCK = 8                                          # SD_GALLERY_BLOCK of skf_chamfer.hip: rows of b per workgroup
SHAPE_MAX_SAMPLES = 16


def shape_distance(xy_a, pen_a, n_a, xy_b, pen_b, n_b, samples_per_segment=4, cross=False):
    """Order-free distances between the ink of sketches (skf_shape_distance_f32; the rule is in include/skf.h): xy (N, T, 2)
    float32, pen (N, T) uint8 and n (N,) int32 as sketch_points returns them (points and pen bytes contiguous in a row; the row
    strides are free), T <= 512.  Every sketch is sampled at its points and at samples_per_segment - 1 interior positions of every
    segment; a sample's distance to the other sketch is that to its nearest dot or segment.  -> float32 (Na, 4), or with
    cross=True (Na, Nb, 4): (mean a->b, mean b->a, max a->b, max b->a).  Chamfer = half the sum of the first two, Hausdorff = the
    larger of the last two.  An empty sketch stands for the single point (0, 0).  Bit-equal to a float32 numpy restatement."""
    for xy, pen, name in ((xy_a, pen_a, "a"), (xy_b, pen_b, "b")):
        if xy.dtype != torch.float32 or xy.dim() != 3 or xy.shape[2] != 2:
            raise TypeError("xy_%s must be a float32 tensor of shape (N, T, 2)" % name)
        if xy.stride(2) != 1 or (xy.shape[1] > 1 and xy.stride(1) != 2) or (xy.shape[0] > 1 and xy.stride(0) < 2 * xy.shape[1]):
            raise ValueError("xy_%s must hold contiguous (x, y) points in rows that do not overlap" % name)
        if pen.dtype != torch.uint8 or tuple(pen.shape) != tuple(xy.shape[:2]) or pen.device != xy.device:
            raise TypeError("pen_%s must be a uint8 tensor of shape (N, T) on the device of xy_%s" % (name, name))
        if (pen.shape[1] > 1 and pen.stride(1) != 1) or (pen.shape[0] > 1 and pen.stride(0) < pen.shape[1]):
            raise ValueError("pen_%s must hold contiguous bytes in rows that do not overlap" % name)
    if xy_b.device != xy_a.device:
        raise ValueError("xy_a and xy_b must be on one device")
    S = int(samples_per_segment)
    if S != samples_per_segment or S < 1 or S > SHAPE_MAX_SAMPLES:
        raise ValueError("samples_per_segment must be an integer in [1, %d] (got %r)" % (SHAPE_MAX_SAMPLES, samples_per_segment))
    (Na, Ta), (Nb, Tb) = xy_a.shape[:2], xy_b.shape[:2]
    _align_lengths(n_a, "n_a", Na, xy_a.device); _align_lengths(n_b, "n_b", Nb, xy_a.device)
    _align_check(Na, Nb, Ta, Tb, cross)
    if cross and Na * Nb * 4 >= 1 << 31:
        raise ValueError("a cross matrix holds fewer than 2^31 floats (got %d x %d x 4): walk the gallery in slabs" % (Na, Nb))
    _p(xy_a); _p(pen_a); _p(xy_b); _p(pen_b); _p(n_a); _p(n_b)   # CPU tensors: SkfError before anything is allocated
    out = torch.empty((Na, Nb, 4) if cross else (Na, 4), dtype=torch.float32, device=xy_a.device)
    _lib.call("skf_shape_distance_f32", _p(xy_a), max(xy_a.stride(0), 2 * Ta), _p(pen_a), max(pen_a.stride(0), Ta), _p(n_a), Na, Ta,
              _p(xy_b), max(xy_b.stride(0), 2 * Tb), _p(pen_b), max(pen_b.stride(0), Tb), _p(n_b), Nb, Tb, S, 1 if cross else 0,
              _p(out), _stream())
    return out


def sequence_score(logits, target, eos, tgt_off=0, T=None):
    """Teacher-forced scoring of given sequences (skf_sequence_score; the rule is in include/skf.h).  logits: float32 or bfloat16,
    (B, T, V), or (B * T, V) with ``T`` given, unit innermost stride; the row pitch may exceed V as long as it is the same for every
    row (a view such as TrainEngine.buffer('logits') is taken as it is - nothing is copied).  target: (B, >= tgt_off + T) int64, row b
    holds the token of position t at column tgt_off + t; eos: the token that ends a sequence.
    -> (tok_logp (B, T) float32, tok_rank (B, T) int32, seq_logp (B,) float32, seq_len (B,) int32) on the device: log p and rank of
    every position in front of the sequence's end (0.0 / -1 behind it, where the logits are not read), their sum in ascending
    order, and the scored length (through the EOS; to the first PAD without one)."""
    if not torch.is_tensor(logits) or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("logits must be a float32 or bfloat16 tensor (got %s)" % (getattr(logits, "dtype", type(logits)),))
    if logits.dim() == 3:
        if T is not None and int(T) != logits.shape[1]:
            raise ValueError("T=%r does not match logits of shape %r" % (T, tuple(logits.shape)))
        B, T, V = logits.shape
        ld = logits.stride(1)
        if logits.stride(2) != 1 or ld < V or (B > 1 and logits.stride(0) != T * ld):
            raise ValueError("logits must have a unit innermost stride and one row pitch >= V for all B * T rows")
    elif logits.dim() == 2:
        if T is None or int(T) < 1 or logits.shape[0] % int(T):
            raise ValueError("logits of shape (B * T, V) need T, a divisor of the row count (got T=%r for %d rows)" % (T, logits.shape[0]))
        T, V = int(T), logits.shape[1]
        B = logits.shape[0] // T
        ld = logits.stride(0) if logits.shape[0] > 1 else V
        if logits.stride(1) != 1 or ld < V:
            raise ValueError("logits must have a unit innermost stride and a row pitch >= V")
    else:
        raise ValueError("logits must have shape (B, T, V), or (B * T, V) with T given")
    if B < 1 or T < 1 or V < 1:
        raise ValueError("logits must hold at least one row and one column")
    tgt_off = int(tgt_off)
    if not torch.is_tensor(target) or target.dtype != torch.int64 or target.dim() != 2:
        raise ValueError("target must be an int64 tensor of shape (B, >= tgt_off + T)")
    if target.device != logits.device:
        raise ValueError("target must be on the device of logits")
    if tgt_off < 0 or target.shape[0] != B or target.shape[1] < tgt_off + T:
        raise ValueError("target must hold B=%d rows of at least tgt_off + T = %d columns (got %r)" % (B, tgt_off + T, tuple(target.shape)))
    if target.stride(1) != 1 or (B > 1 and target.stride(0) < target.shape[1]):
        raise ValueError("target must have a unit innermost stride and rows that do not overlap")
    _p(logits); _p(target)                                       # CPU tensors: SkfError before anything is allocated
    dev = logits.device
    f32 = torch.empty(B * (T + 1), dtype=torch.float32, device=dev)      # two allocations for the four results
    i32 = torch.empty(B * (T + 1), dtype=torch.int32, device=dev)
    tok_logp, seq_logp, tok_rank, seq_len = f32[:B * T].view(B, T), f32[B * T:], i32[:B * T].view(B, T), i32[B * T:]
    _lib.call("skf_sequence_score", _p(logits), int(logits.dtype == torch.bfloat16), ld, B, T, V, _p(target),
              max(target.stride(0), target.shape[1]), tgt_off, int(eos), _p(tok_logp), _p(tok_rank), _p(seq_logp), _p(seq_len), _stream())
    return tok_logp, tok_rank, seq_logp, seq_len
