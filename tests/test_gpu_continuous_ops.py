"""The continuous stroke-5 stage (skf_continuous.hip) through the C ABI, entry point by entry point, against float64 - at the sizes
where its grid caps, the second trip of its grid-stride loops and the one-workgroup reductions are reached (the model-level test runs
about 120 rows).  Bars as in tests/test_gpu_ops.py: 2e-5 of the tensor's maximum element-wise, 5e-5 for sums over rows.  Every output
buffer is filled with a sentinel first; cells outside the documented output keep it."""
import numpy as np
import pytest
import torch

import entry_point_checks as epc
import oracle
from entry_point_checks import SENTINEL, close, dev, filled, ptr, stream

pytestmark = pytest.mark.gpu
ELT_RTOL, SUM_RTOL = 2e-5, 5e-5


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    epc.report()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _step_state(seed):
    from sketchformer_amd import ops
    st = ops.new_step_state("cuda", iterations=3)
    ops.step_prologue(st, seed=seed)
    return st, ops.read_step_state(st)["drop_key"]


def _keep(key, site, rate, rows, d):
    from sketchformer_amd import ops
    if rate == 0:
        return None
    return ops.dropout_keep_mask(key, site, rate, rows * d).reshape(rows, d)


# ------------------------------------------------------------------ skf_padding_mask_continuous
@pytest.mark.parametrize("B,L,ld_rows", [pytest.param(3, 7, 9, id="3x7-one-workgroup"),
                                         pytest.param(513, 512, 513, id="513x512-grid-cap-1024-second-trip")])
def test_padding_mask_continuous(lib, B, L, ld_rows):
    rng = np.random.RandomState(B)
    x = rng.randn(B, ld_rows, 5).astype(np.float32)
    pen = np.array([1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0], np.float32)      # only exactly 1.0 masks
    x[:, :, 4] = pen[rng.randint(0, 3, size=(B, ld_rows))]
    x[0, :3, 4] = pen
    X = dev(x)
    out = filled(B * L + 8, dtype=torch.uint8, value=0xAB)
    lib.call("skf_padding_mask_continuous", ptr(X), ld_rows, B, L, ptr(out), stream())
    got = out.cpu().numpy()
    assert np.array_equal(got[:B * L].reshape(B, L), (x[:, :L, 4] == np.float32(1.0)).astype(np.uint8))
    assert list(got[:3]) == [1, 0, 0] and (got[B * L:] == 0xAB).all()


# ------------------------------------------------------------------ skf_embed_continuous_fwd / _bwd
EMBED_ROWS = [pytest.param(1, 7, id="rows7-two-workgroups"), pytest.param(33, 250, id="rows8250-grid-caps-second-trip")]


def _embed_inputs(B, L, d, seed):
    rng = np.random.RandomState(seed)
    x = _f32(rng.uniform(0.25, 1.0, (B, L + 1, 5)))                   # x_ld_rows = L + 1: the last row of a sample is never read
    W, bias, pos = _f32(rng.uniform(-1, 1, (5, d))), _f32(rng.uniform(-1, 1, d)), _f32(rng.uniform(-1, 1, (L, d)))
    return rng, x, W, bias, pos


@pytest.mark.parametrize("rate", [pytest.param(0.0, id="no-dropout"), pytest.param(0.1, id="dropout")])
@pytest.mark.parametrize("d", [pytest.param(36, id="d36-partial-wave"), pytest.param(64, id="d64-one-column-trip"),
                               pytest.param(200, id="d200-four-column-trips")])
@pytest.mark.parametrize("B,L", EMBED_ROWS)
def test_embed_continuous_fwd(lib, B, L, d, rate):
    rows, site = B * L, 5
    _, x, W, bias, pos = _embed_inputs(B, L, d, rows + d)
    st, key = _step_state(seed=d)
    X, Wd, bd, pd = dev(x), dev(W), dev(bias), dev(pos)
    out = filled(rows * d + 7)
    lib.call("skf_embed_continuous_fwd", ptr(X), L + 1, B, L, ptr(Wd), ptr(bd), d, ptr(pd), ptr(out), rate, site, ptr(st), stream())
    want = ((x[:, :L] @ W + bias) * np.sqrt(d) + pos[None]).reshape(rows, d)
    want = oracle.dropout_fwd(want, _keep(key, site, rate, rows, d), rate)
    close(out[:rows * d].view(rows, d), want, ELT_RTOL, "skf_embed_continuous_fwd", "out")
    assert float(out[rows * d:].min()) == float(out[rows * d:].max()) == SENTINEL


def _embed_bwd(lib, B, L, d, rate, short_by=0):
    rows, site = B * L, 6
    rng, x, _, _, _ = _embed_inputs(B, L, d, rows + d + 1)
    dx = _f32(rng.uniform(0.25, 1.0, (rows, d)) * np.where(rng.rand(d) < 0.5, -1.0, 1.0))    # one sign per column: no cancellation
    st, key = _step_state(seed=d + 1)
    X, DX = dev(x), dev(dx)
    nbytes = lib.load().skf_embed_continuous_bwd_workspace_bytes(rows, d)
    assert nbytes == min((rows + 3) // 4, 256) * 6 * d * 4
    ws = filled(nbytes // 4 + 4)
    dW, db = filled(5 * d + 3), filled(d + 3)
    lib.call("skf_embed_continuous_bwd", ptr(X), L + 1, B, L, ptr(DX), d, ptr(dW), ptr(db), rate, site, ptr(st), ptr(ws),
             nbytes - short_by, stream())
    g = oracle.dropout_fwd(dx, _keep(key, site, rate, rows, d), rate) * np.sqrt(d)
    close(dW[:5 * d].view(5, d), x[:, :L].reshape(rows, 5).T @ g, SUM_RTOL, "skf_embed_continuous_bwd", "dW")
    close(db[:d], g.sum(0), SUM_RTOL, "skf_embed_continuous_bwd", "dbias")
    for t in (dW[5 * d:], db[d:], ws[nbytes // 4:]):
        assert float(t.min()) == float(t.max()) == SENTINEL


@pytest.mark.parametrize("rate", [pytest.param(0.0, id="no-dropout"), pytest.param(0.1, id="dropout")])
@pytest.mark.parametrize("d", [pytest.param(36, id="d36-partial-wave"), pytest.param(64, id="d64-one-column-trip"),
                               pytest.param(200, id="d200-four-column-trips")])
@pytest.mark.parametrize("B,L", [pytest.param(1, 7, id="rows7-two-partial-rows-idle-colsum-groups"),
                                 pytest.param(33, 250, id="rows8250-grid-cap-256-sixteen-partials-per-group")])
def test_embed_continuous_bwd(lib, B, L, d, rate):
    _embed_bwd(lib, B, L, d, rate)


def test_embed_continuous_bwd_widest_d_and_refusals(lib):
    """d = 640 is the widest multiple of 64 whose [4 waves][6][d] floats fit 64 KB of LDS (d <= 682); 704 is refused, and so is a
    workspace one float short of skf_embed_continuous_bwd_workspace_bytes."""
    _embed_bwd(lib, 1, 7, 640, 0.0)
    with pytest.raises(lib.SkfError, match="d_model too large"):
        _embed_bwd(lib, 1, 7, 704, 0.0)
    with pytest.raises(lib.SkfError, match="workspace too small"):
        _embed_bwd(lib, 1, 7, 64, 0.0, short_by=4)


# ------------------------------------------------------------------ skf_continuous_loss
ONE_HOT = np.eye(3)
TIES = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 1.0, 1.0]])         # first index wins: labels 0, 0, 1 (the last is a padded row)


def _loss_inputs(B, cols, ld_rows, off, seed, all_padding=False):
    rng = np.random.RandomState(seed)
    tgt = np.zeros((B, ld_rows, 5))
    tgt[..., :2] = rng.randn(B, ld_rows, 2)
    tgt[..., 2:] = ONE_HOT[rng.choice(3, size=(B, ld_rows), p=[0.6, 0.25, 0.15])]
    tgt[0, off:off + 3, 2:] = TIES
    if B > 1:
        tgt[1, :, 2:] = ONE_HOT[2]                                            # one sample that is all padding
    if all_padding:
        tgt[..., 2:] = ONE_HOT[2]
    pred = np.zeros((B, cols, 5))
    pred[..., :2] = rng.randn(B, cols, 2)
    pred[..., 2:] = 2.0 * rng.randn(B, cols, 3)
    extreme = np.zeros((B, cols), bool)
    extreme[-1, -4:] = True
    pred[-1, -4:, 2:] = np.array([[80, -80, 0], [-80, 80, -80], [-80, -80, 80], [80, 80, -80]])[-min(4, cols):]
    return _f32(tgt), _f32(pred), extreme.reshape(-1)


def _run_loss(lib, pred, tgt, ld_rows, cols, off, weight, write_grad):
    rows = pred.shape[0] * pred.shape[1]
    P = filled(rows * 5 + 5)
    P[:rows * 5] = dev(pred.reshape(-1))
    T = dev(tgt)
    loc, ce, mask, scal = filled(rows + 3), filled(rows + 3), filled(rows + 3), filled(8)
    lib.call("skf_continuous_loss", ptr(P), ptr(T), ld_rows, cols, off, rows, weight, ptr(loc), ptr(ce), ptr(mask), ptr(scal), write_grad,
             stream())
    for t, n in ((P, rows * 5), (loc, rows), (ce, rows), (mask, rows), (scal, 4)):
        assert float(t[n:].min()) == float(t[n:].max()) == SENTINEL
    return P[:rows * 5].view(rows, 5), loc[:rows], ce[:rows], mask[:rows], scal[:4]


@pytest.mark.parametrize("weight", [pytest.param(1.0, id="w1"), pytest.param(0.25, id="w0.25")])
@pytest.mark.parametrize("B,cols,ld_rows,off", [
    pytest.param(3, 5, 6, 1, id="rows15-one-workgroup"),
    pytest.param(4, 129, 130, 1, id="rows516-three-workgroups-reduce-second-trip"),
    pytest.param(513, 512, 513, 1, id="rows262656-grid-cap-1024-second-trip")])
def test_continuous_loss(lib, B, cols, ld_rows, off, weight):
    tgt, pred, extreme = _loss_inputs(B, cols, ld_rows, off, seed=B + cols)
    rows = B * cols
    real = tgt[:, off:off + cols]
    want_loss, cache = oracle.continuous_recon_loss_fwd(real, pred, weight)
    want_g = oracle.continuous_recon_loss_bwd(cache).reshape(rows, 5)
    _, _, w_mask, lab, lsm, _ = cache
    assert list(lab[0, :3]) == [0, 0, 1] and w_mask[0, 2] == 0.0              # the tie rows: first index; (0,1,1) is a padded row
    w_loc = ((real[..., :2] - pred[..., :2]) ** 2).mean(-1).reshape(-1)
    w_ce = -np.take_along_axis(lsm, lab[..., None], -1).reshape(-1)
    # forward only: pred is left alone, bit for bit
    P0, loc, ce, mask, scal = _run_loss(lib, pred, tgt, ld_rows, cols, off, weight, 0)
    assert torch.equal(P0.cpu(), torch.as_tensor(pred.reshape(rows, 5), dtype=torch.float32))
    G, loc1, ce1, mask1, scal1 = _run_loss(lib, pred, tgt, ld_rows, cols, off, weight, 1)
    for a, b in ((loc, loc1), (ce, ce1), (mask, mask1), (scal, scal1)):
        assert torch.equal(a, b)
    close(loc, w_loc, ELT_RTOL, "skf_continuous_loss", "row_loc")
    ex = torch.as_tensor(extreme).cuda()
    close(ce[~ex], w_ce[~extreme], ELT_RTOL, "skf_continuous_loss", "row_ce")
    close(ce[ex], w_ce[extreme], ELT_RTOL, "skf_continuous_loss", "row_ce (logits +-80)")
    assert np.array_equal(epc.host64(mask), w_mask.reshape(-1))
    assert float(mask.view(B, cols)[1].abs().max() if B > 1 else 0.0) == 0.0
    close(scal[0:1], [(w_loc * w_mask.reshape(-1)).sum()], SUM_RTOL, "skf_continuous_loss", "sum(loc*mask)")
    close(scal[1:2], [w_ce.sum()], SUM_RTOL, "skf_continuous_loss", "sum(ce)")
    assert float(scal[2]) == w_mask.sum()
    close(scal[3:4], [want_loss], SUM_RTOL, "skf_continuous_loss", "loss")
    close(G[:, :2], want_g[:, :2], ELT_RTOL, "skf_continuous_loss", "grad location")
    close(G[:, 2:], want_g[:, 2:], ELT_RTOL, "skf_continuous_loss", "grad pen logits")
    dead = torch.as_tensor(w_mask.reshape(-1) == 0).cuda()
    assert float(G[dead][:, :2].abs().max()) == 0.0                             # padded rows: no location gradient at all


def test_continuous_loss_batch_of_padding_only(lib):
    B, cols, ld_rows, off = 3, 5, 6, 1
    tgt, pred, _ = _loss_inputs(B, cols, ld_rows, off, seed=4, all_padding=True)
    G, loc, ce, mask, scal = _run_loss(lib, pred, tgt, ld_rows, cols, off, 1.0, 1)
    assert float(mask.abs().max()) == 0.0
    assert float(scal[0]) == 0.0 and float(scal[2]) == 0.0 and float(scal[3]) == 0.0       # the loss is exactly 0
    assert float(scal[1]) > 0.0
    assert float(G.abs().max()) == 0.0                                                       # pen-logit (and location) gradient exactly 0
