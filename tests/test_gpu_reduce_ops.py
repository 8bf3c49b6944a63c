"""The reduction hub through the C ABI, against float64: skf_colsum, skf_splitk_reduce, skf_splitk_reduce_batch (one launch that sums
every weight-gradient slab, LayerNorm dgamma|dbeta partial and expander / pooling partial of a train step) and skf_metrics_update.
Inputs are positive (times a sign per column), so no expected sum is a near-cancellation; the bar is the 5e-5 that
tests/test_gpu_ops.py uses for results that sum over rows.  Every output buffer is filled with a sentinel first."""
import ctypes as C

import numpy as np
import pytest
import torch

import entry_point_checks as epc
from entry_point_checks import SENTINEL, close, dev, filled, ptr, stream

pytestmark = pytest.mark.gpu
SUM_RTOL = 5e-5


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    epc.report()


def _signed(rng, *shape):
    """values in +-[0.25, 1], one sign per last-axis column: sums over the leading axes never cancel"""
    return rng.uniform(0.25, 1.0, shape) * np.where(rng.rand(shape[-1]) < 0.5, -1.0, 1.0)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------ skf_colsum
@pytest.mark.parametrize("ncols", [pytest.param(1, id="cols1"), pytest.param(63, id="cols63-partial-block"),
                                   pytest.param(64, id="cols64-one-block"), pytest.param(65, id="cols65-second-block"),
                                   pytest.param(200, id="cols200-four-blocks")])
@pytest.mark.parametrize("nrows", [pytest.param(1, id="rows1"), pytest.param(15, id="rows15-idle-group"),
                                   pytest.param(16, id="rows16-one-per-group"), pytest.param(17, id="rows17-second-trip"),
                                   pytest.param(63, id="rows63-tail-only"), pytest.param(64, id="rows64-tail-only-full"),
                                   pytest.param(65, id="rows65-unrolled-once"), pytest.param(640, id="rows640-unrolled-ten")])
def test_colsum(lib, nrows, ncols):
    rng = np.random.RandomState(1000 * nrows + ncols)
    ld = ncols + 3
    a = _f32(_signed(rng, nrows, ld))
    A = dev(a)
    out0 = _f32(rng.uniform(0.25, 1.0, ncols) * np.sign(a[0, :ncols]))
    for accumulate in (0, 1):
        out = filled(ncols + 5)
        if accumulate:
            out[:ncols] = dev(out0)
        lib.call("skf_colsum", ptr(A), nrows, ld, ncols, ptr(out), accumulate, stream())
        want = a[:, :ncols].sum(0) + (out0 if accumulate else 0.0)
        close(out[:ncols], want, SUM_RTOL, "skf_colsum", "sum")
        assert float(out[ncols:].min()) == float(out[ncols:].max()) == SENTINEL       # the pad columns of `in` are never summed


# ------------------------------------------------------------------ skf_splitk_reduce
SHAPES = [pytest.param(4, 3, id="4x3-scalar-path"), pytest.param(5, 8, id="5x8-vector-path"),
          pytest.param(8, 64, id="8x64-vector-path-two-blocks"), pytest.param(64, 345, id="64x345-scalar-path")]
SPLITS = [pytest.param(1, id="splits1"), pytest.param(3, id="splits3-idle-group"), pytest.param(4, id="splits4-one-per-group"),
          pytest.param(5, id="splits5-tail-twice"), pytest.param(16, id="splits16-unrolled-once"),
          pytest.param(17, id="splits17-unrolled-then-tail"), pytest.param(29, id="splits29-unrolled-one-group-only")]


def _slab(rng, splits, M, N, bias, slack=0):
    """[splits][M][N] tiles then (bias) [splits][N] column sums, `slack` floats of 1e30 behind: (device slab, tiles64, colsums64)"""
    tiles = _f32(_signed(rng, splits, M, N))
    cs = _f32(_signed(rng, splits, N)) if bias else None
    flat = np.concatenate([tiles.reshape(-1)] + ([cs.reshape(-1)] if bias else []) + [np.full(slack, 1e30)])
    return dev(flat), tiles, cs


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("splits", SPLITS)
def test_splitk_reduce(lib, splits, M, N):
    rng = np.random.RandomState(splits * 7919 + M * N)
    ldc = N + 5
    for bias in (False, True):
        slab, tiles, cs = _slab(rng, splits, M, N, bias)
        c0 = _f32(rng.uniform(0.25, 1.0, (M, N)) * np.sign(tiles[0, :1, :]))
        b0 = _f32(rng.uniform(0.25, 1.0, N) * np.sign(cs[0])) if bias else None
        for accumulate in (0, 1):
            Cd = filled(M, ldc)
            bg = filled(N + 3) if bias else None
            if accumulate:
                Cd[:, :N] = dev(c0)
                if bias:
                    bg[:N] = dev(b0)
            lib.call("skf_splitk_reduce", ptr(slab), splits, M, N, ptr(Cd), ldc, accumulate, ptr(bg), accumulate, stream())
            close(Cd[:, :N], tiles.sum(0) + (c0 if accumulate else 0.0), SUM_RTOL, "skf_splitk_reduce", "C")
            assert float(Cd[:, N:].min()) == float(Cd[:, N:].max()) == SENTINEL
            if bias:
                close(bg[:N], cs.sum(0) + (b0 if accumulate else 0.0), SUM_RTOL, "skf_splitk_reduce", "bias_grad")
                assert float(bg[N:].min()) == float(bg[N:].max()) == SENTINEL


def test_splitk_reduce_refuses_a_tile_that_is_no_multiple_of_four(lib):
    slab = torch.zeros(64, device="cuda")
    Cd = filled(3, 8)
    for M, N, offset in ((3, 3, 0), (1, 5, 0), (3, 6, 0), (2, 4, 4)):        # the last: M*N fine, slab not 16-byte aligned
        with pytest.raises(lib.SkfError):
            lib.call("skf_splitk_reduce", ptr(slab, offset), 2, M, N, ptr(Cd), 8, 0, None, 0, stream())
    torch.cuda.synchronize()
    assert float(Cd.min()) == float(Cd.max()) == SENTINEL


# ------------------------------------------------------------------ skf_splitk_reduce_batch
def test_splitk_reduce_batch_six_descriptors_one_launch(lib):
    """The four shapes of the single-slab test with a bias gradient (M*N % 4 == 0 in all of them, as the contract of SkfReduceDesc asks),
    the expander's 1 x 199 partials and the LayerNorm form 1 x 256 with 640 splits.  Behind every slab whose last float4 group is read
    beyond the data (1 x 199: M*N % 4 != 0; 4 x 3 and 64 x 345: N % 4 != 0 in the column sums) lie 16 bytes of 1e30: read, never summed."""
    l = lib.load()
    rng = np.random.RandomState(77)
    forms = [("4x3-bias", 4, 3, 3, True), ("5x8-bias", 5, 8, 17, True), ("8x64-bias", 8, 64, 16, True), ("64x345-bias", 64, 345, 29, True),
             ("1x199-expander", 1, 199, 5, False), ("1x256-layernorm", 1, 256, 640, False)]
    descs = (lib.SkfReduceDesc * len(forms))()
    keep, begin = [], 0
    for i, (name, M, N, splits, bias) in enumerate(forms):
        slab, tiles, cs = _slab(rng, splits, M, N, bias, slack=4)
        ldc = N + 5
        Cd, bg = filled(M, ldc), (filled(N + 3) if bias else None)
        assert slab.data_ptr() % 16 == 0
        d = descs[i]
        d.slab, d.C, d.bias_grad = slab.data_ptr(), Cd.data_ptr(), (bg.data_ptr() if bias else None)
        d.splits, d.M, d.N, d.ldc, d.block_begin, d.pad = splits, M, N, ldc, begin, 0
        begin += l.skf_splitk_reduce_blocks(M, N)
        keep.append((name, M, N, splits, bias, slab, tiles, cs, Cd, bg))
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    lib.call("skf_splitk_reduce_batch", ptr(table), len(forms), begin, stream())
    for name, M, N, splits, bias, slab, tiles, cs, Cd, bg in keep:
        close(Cd[:, :N], tiles.sum(0), SUM_RTOL, "skf_splitk_reduce_batch", "C")
        assert float(Cd[:, N:].min()) == float(Cd[:, N:].max()) == SENTINEL, name
        if bias:
            close(bg[:N], cs.sum(0), SUM_RTOL, "skf_splitk_reduce_batch", "bias_grad")
            assert float(bg[N:].min()) == float(bg[N:].max()) == SENTINEL, name
        if N % 4 == 0:                                       # the single-slab call takes its float4 path: same adds in the same order
            C1, b1 = filled(M, N + 5), (filled(N + 3) if bias else None)
            lib.call("skf_splitk_reduce", ptr(slab), splits, M, N, ptr(C1), N + 5, 0, ptr(b1), 0, stream())
            assert torch.equal(C1, Cd), name
            assert not bias or torch.equal(b1, bg), name


# ------------------------------------------------------------------ skf_metrics_update
@pytest.mark.parametrize("class_rows", [pytest.param(0, id="no-class-head"), pytest.param(7, id="class7")])
@pytest.mark.parametrize("offset", [pytest.param(0, id="aligned-float4"), pytest.param(4, id="offset4-scalar")])
@pytest.mark.parametrize("recon_rows", [pytest.param(3, id="rows3-tail-only"), pytest.param(4, id="rows4-one-float4"),
                                        pytest.param(4097, id="rows4097-1024-float4-and-tail"),
                                        pytest.param(25472, id="rows25472-second-sweep")])
def test_metrics_update_two_calls(lib, recon_rows, offset, class_rows):
    rng = np.random.RandomState(recon_rows + class_rows)
    rw, cw = 0.75, 1.5
    m = filled(32)
    m[8:13] = 0.0
    m[16:21] = 0.0
    tot, cnt = np.zeros(5), np.zeros(5)
    for call in range(2):
        rl, rh = _f32(rng.uniform(0.1, 2.0, recon_rows)), (rng.rand(recon_rows) < 0.4).astype(np.float64)
        cl, ch = _f32(rng.uniform(0.1, 2.0, class_rows)), (rng.rand(class_rows) < 0.6).astype(np.float64)
        lead = [1e30] * (offset // 4)                                                # neighbours that must not be summed
        RL, RH = (dev(np.concatenate([lead, v, [1e30]]))[len(lead):] for v in (rl, rh))
        assert RL.data_ptr() % 16 == offset and RH.data_ptr() % 16 == offset         # offset 4: the scalar loop, no float4 load
        CL, CH = (dev(cl), dev(ch)) if class_rows else (None, None)
        lib.call("skf_metrics_update", ptr(RL), ptr(RH), recon_rows, rw, ptr(CL), ptr(CH), class_rows, cw, None, ptr(m), stream())
        r_loss, c_loss = rw * rl.sum() / recon_rows, (cw * cl.sum() / class_rows if class_rows else 0.0)
        step = np.array([r_loss, rh.sum() / recon_rows, c_loss, ch.sum() / class_rows if class_rows else 0.0, r_loss + c_loss])
        tot += [r_loss, rh.sum(), c_loss, ch.sum(), r_loss + c_loss]
        cnt += [1, recon_rows, 1, class_rows, 1]
        got = epc.host64(m)
        close(got[0:5], step, SUM_RTOL, "skf_metrics_update", "step")
        close(got[8:13], tot, SUM_RTOL, "skf_metrics_update", "totals")
        assert np.array_equal(got[16:21], cnt)
        assert got[9] == tot[1] and got[11] == tot[3]                                 # hit counts are whole numbers < 2^24: exact
        assert (np.delete(got, list(range(0, 5)) + list(range(8, 13)) + list(range(16, 21))) == SENTINEL).all()


def test_metrics_update_recon_scalar_form(lib):
    """Continuous mode hands over the already reduced reconstruction loss: no token accuracy, its count does not advance."""
    rng = np.random.RandomState(5)
    m = filled(32)
    m[8:13] = 0.0
    m[16:21] = 0.0
    rl, rh = dev(rng.uniform(0.1, 2.0, 8)), dev(np.ones(8))
    cl, ch = _f32(rng.uniform(0.1, 2.0, 7)), (rng.rand(7) < 0.6).astype(np.float64)
    CL, CH = dev(cl), dev(ch)
    scal = dev([0.8125])
    for call in (1, 2):
        lib.call("skf_metrics_update", ptr(rl), ptr(rh), 8, 0.75, ptr(CL), ptr(CH), 7, 1.5, ptr(scal), ptr(m), stream())
        got = epc.host64(m)
        c_loss = 1.5 * cl.sum() / 7
        close(got[0:5], np.array([0.8125, 0.0, c_loss, ch.sum() / 7, 0.8125 + c_loss]), SUM_RTOL, "skf_metrics_update", "step (recon_scalar)")
        assert got[1] == 0.0 and got[9] == 0.0 and got[17] == 0.0
        close(got[8:13], call * np.array([0.8125, 0.0, c_loss, ch.sum(), 0.8125 + c_loss]), SUM_RTOL, "skf_metrics_update", "totals (recon_scalar)")
        assert np.array_equal(got[16:21], [call, 0, call, 7 * call, call])
