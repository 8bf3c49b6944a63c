"""The key-mask scan that opens the head-size-16 attention kernels (split arithmetic): which key tiles hold a padded key, the last
un-padded key, whether key 0 is visible.  Forward (skf_attention.hip) and one-pass backward (skf_attention_bwd3.hip) form all of
it from wave ballots of the mask bytes; the cases below sit on every edge of that scan - key counts on, one past and one short of
a 16-key tile and a 64-key wave, the longest sequence the backward kernel takes, masks that set none, all, the first, all but the
last and every other key, and padded tails that end on and off a tile edge - against the oracle at the tolerances
tests/test_gpu_ops.py uses for masked attention (fp32 oracle: a fully masked row is uniform only in fp32)."""
import numpy as np
import pytest
import torch

import oracle
from sketchformer_amd import _lib

pytestmark = pytest.mark.gpu

B, H, DH = 2, 2, 16
LENGTHS = [16, 17, 63, 64, 65, 199, 208]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _split(x):
    b, L, d = x.shape
    return x.reshape(b, L, H, d // H).transpose(0, 2, 1, 3).astype(np.float32)


def _merge(x):
    b, h, L, dh = x.shape
    return x.transpose(0, 2, 1, 3).reshape(b, L, h * dh)


def _close(got, want, rtol, name, floor=1e-30):
    got = got.detach().cpu().numpy().astype(np.float64)
    want = np.asarray(want, np.float64)
    assert np.isfinite(got).all(), name + ": non-finite output"
    scale = max(np.abs(want).max(), floor)
    err = np.abs(got - want).max() / scale
    assert err <= rtol, "%s: rel err %.3e > %.1e" % (name, err, rtol)


def _masks(Lk):
    """name -> (B, Lk) bool key mask (True = padded) or None"""
    keys = np.arange(Lk)
    edge = 16 * ((Lk - 1) // 16) or 16             # a valid length that ends on a tile edge (Lk = 16: nothing padded)
    tail = lambda lens: keys[None, :] >= np.asarray(lens)[:, None]
    first = np.zeros((B, Lk), bool); first[:, 0] = True
    last = np.ones((B, Lk), bool); last[:, Lk - 1] = False
    return {
        "none": None,
        "zeros": np.zeros((B, Lk), bool),
        "all": np.ones((B, Lk), bool),
        "key0": first,                                                   # causal tile skipping off
        "last_only": last,
        "alternating": np.stack([keys % 2 == 1, keys % 2 == 0]),         # (sample 1 also hides key 0)
        "tail": tail([edge, max(1, edge - 5)]),                          # on / off a tile edge
        "tail_short": tail([max(1, Lk // 3), 16 * (Lk // 32) or 1]),
    }


@pytest.mark.parametrize("precision", [_lib.PREC_BF16X6, _lib.PREC_F32])
@pytest.mark.parametrize("Lk", [257, 320, 500])
def test_attention_forward_mask_scan_in_several_passes(Lk, precision):
    """More than 256 keys (the forward kernel's long form, with and without split arithmetic): a thread scans a key in each of two
    passes; padded tails that end in the first pass, on the pass edge and in the second, a hole, and a fully padded sample."""
    from sketchformer_amd import ops
    nb, Lq, d = 5, 40, H * DH
    rng = np.random.RandomState(Lk)
    q, k, v = rng.randn(nb, Lq, d), rng.randn(nb, Lk, d), rng.randn(nb, Lk, d)
    km = np.arange(Lk)[None, :] >= np.array([Lk, 100, 256, Lk - 3, 0])[:, None]
    km[0, 250:270] = True
    km[3, 0] = True
    want_o, _, _ = oracle.sdpa_fwd(_split(q), _split(k), _split(v), km[:, None, None, :].astype(np.float32))
    o, _ = ops.attention_fwd(_dev(q), _dev(k), _dev(v), H, key_mask=_dev(km, torch.uint8), precision=precision)
    _close(o, _merge(want_o), 1e-4, "fwd Lk %d" % Lk)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Lk", LENGTHS)
def test_attention_mask_scan_edges(Lk, causal):
    from sketchformer_amd import ops
    Lq, d = Lk, H * DH
    rng = np.random.RandomState(7 * Lk + int(causal))
    q, k, v, do = (rng.randn(B, L, d) for L in (Lq, Lk, Lk, Lq))
    live = np.array([max(1, Lq // 2), Lq], np.int32)
    do_live = do * (np.arange(Lq)[None, :, None] < live[:, None, None])
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    for name, km in _masks(Lk).items():
        mask = np.zeros((B, 1, Lq, Lk), np.float32)
        if km is not None:
            mask = np.maximum(mask, km[:, None, None, :].astype(np.float32))
        if causal:
            mask = np.maximum(mask, oracle.create_look_ahead_mask(Lq)[None, None])
        want_o, _, cache = oracle.sdpa_fwd(_split(q), _split(k), _split(v), mask)
        kmd = _dev(km, torch.uint8) if km is not None else None
        o, stats = ops.attention_fwd(qd, kd, vd, H, key_mask=kmd, causal=causal, precision=_lib.PREC_BF16X6)
        tag = "Lk %d causal %d mask %s: " % (Lk, causal, name)
        _close(o, _merge(want_o), 1e-4, tag + "fwd")
        for g_out, ll in ((do, None), (do_live, live)):
            want = oracle.sdpa_bwd(_split(g_out), cache)
            got = ops.attention_bwd(qd, kd, vd, o, _dev(g_out), stats, H, key_mask=kmd, causal=causal, precision=_lib.PREC_BF16X6,
                                    q_live_len=torch.as_tensor(ll).cuda() if ll is not None else None)
            for g, w, n in zip(got, want, ("dQ", "dK", "dV")):
                _close(g, _merge(w), 3e-4, tag + n + (" (q_live)" if ll is not None else ""), floor=0.1)
