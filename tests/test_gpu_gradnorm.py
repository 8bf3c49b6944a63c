"""Gradient norms, clip scales, the in-place segment scale and the sweeps with device-side control on synthetic flat buffers,
against the float64 / float32 restatement of tests/clip_reference.py.

The bound on a norm: |got - want| <= 2^-23 * want.  A sum of n < 2^24 non-negative fp64 terms errs by less than 2^-29 relative
(n * 2^-53), the square root halves that, and the one rounding to fp32 adds at most 2^-24."""
import numpy as np
import pytest
import torch

import clip_reference as R

pytestmark = pytest.mark.gpu

NORM_RTOL = 2.0 ** -23
BIG, BIGN, TOTAL = 332, 2 * R.CHUNK + 5, 33288
# 1x1, 1x3, 5x7; three interleaved 8x12 views (row stride 36: the shape of a fused wq|wk|wv block); three chunks with a ragged last
# one; an all-zero entry; values near 1e25 (their squares overflow fp32) and near 1e-30 (their squares underflow it).  Every entry
# starts on a multiple of 4 floats like the model's; the floats between them belong to no entry.
ENTRIES = [R.entry(0, 1, 1, name="one"), R.entry(4, 1, 3, name="three"), R.entry(8, 5, 7, name="5x7"),
           R.entry(44, 8, 12, 36, name="q"), R.entry(56, 8, 12, 36, name="k"), R.entry(68, 8, 12, 36, name="v"),
           R.entry(BIG, 1, BIGN, name="big"), R.entry(33108, 1, 6, name="zero"), R.entry(33116, 3, 40, name="huge"),
           R.entry(33236, 1, 50, name="tiny")]


def _host_buffer():
    rng = np.random.RandomState(7)
    flat = np.full(TOTAL, np.nan, dtype=np.float32)             # the gaps hold NaN: a kernel that reads one shows it
    for e in ENTRIES:
        v = R.view(flat, e)
        v[...] = rng.randn(e["rows"], e["cols"]).astype(np.float32)
        if e["name"] == "zero":
            v[...] = 0.0
        elif e["name"] == "huge":
            v[...] *= np.float32(1e25)
        elif e["name"] == "tiny":
            v[...] *= np.float32(1e-30)
    return flat


def _gap_mask():
    used = np.zeros(TOTAL, dtype=bool)
    for e in ENTRIES:
        R.view(used, e)[...] = True
    return ~used


@pytest.fixture(scope="module")
def case():
    from sketchformer_amd import ops
    host = _host_buffer()
    assert R.n_chunks(ENTRIES) == 12 and _gap_mask().sum() > 0 and np.isnan(host[_gap_mask()]).all()
    per, glob = R.norms(host, ENTRIES)
    return {"ops": ops, "host": host, "flat": torch.from_numpy(host).cuda(), "plan": ops.segment_plan(ENTRIES, "cuda"),
            "per": per, "glob": glob}


def _read(case, stats):
    return case["ops"].read_segment_stats(stats, len(ENTRIES))


def test_norms_match_the_float64_restatement_and_gaps_are_not_read(case):
    ops = case["ops"]
    assert case["plan"].n_chunks == 12 and case["plan"].n_entries == len(ENTRIES)
    stats = ops.segment_norms(case["flat"], case["plan"])
    again = ops.segment_norms(case["flat"], case["plan"])
    assert torch.equal(stats.view(torch.int32), again.view(torch.int32))          # two runs: the same bits
    st = _read(case, stats)
    assert st["nonfinite"] == 0 and not st["skipped"] and st["skipped_total"] == 0
    assert np.isfinite(st["norms"]).all() and np.isfinite(st["global_norm"])
    for e, got, want in zip(ENTRIES, st["norms"], case["per"]):
        print("%-6s got %.9g want %.17g rel %.3g" % (e["name"], got, want, abs(got - want) / want if want else 0.0))
        assert abs(float(got) - want) <= NORM_RTOL * want, e["name"]
    assert abs(st["global_norm"] - case["glob"]) <= NORM_RTOL * case["glob"]
    assert st["norms"][7] == 0.0 and st["norms"][8] > 1e25 and 0 < st["norms"][9] < 1e-28
    assert st["scale"] == 1.0 and (st["scales"] == 1.0).all()                       # mode none: norms only
    half = _read(case, ops.segment_norms(case["flat"], case["plan"], grad_scale=0.5))
    assert half["global_norm"] == 0.5 * st["global_norm"] and np.array_equal(half["norms"], 0.5 * st["norms"])      # a factor on the norms
    small = [R.entry(0, 1, 2), R.entry(4, 1, 1)]                                     # 3-4-5 and 5-12-13, exactly
    got = ops.read_segment_stats(ops.segment_norms(torch.tensor([3.0, 4.0, float("nan"), float("nan"), -12.0], device="cuda"),
                                                   ops.segment_plan(small, "cuda")))
    assert got["norms"].tolist() == [5.0, 12.0] and got["global_norm"] == 13.0


@pytest.mark.parametrize("mode", ["global", "per_variable"])
def test_scales_are_the_restatement_on_the_devices_own_norms(case, mode):
    ops = case["ops"]
    base = _read(case, ops.segment_norms(case["flat"], case["plan"]))
    thresholds = [float(np.median(base["norms"])), float(base["global_norm"]), float(base["norms"][2]), 2.0 * float(base["global_norm"])]
    for c in thresholds:                                       # a median, the norm == c boundaries, and nothing to clip
        st = _read(case, ops.segment_norms(case["flat"], case["plan"], mode=mode, threshold=c))
        assert np.array_equal(st["norms"], base["norms"]) and st["global_norm"] == base["global_norm"]
        g, per = R.scales(st["norms"], np.float32(st["global_norm"]), mode, c)
        assert np.float32(st["scale"]).tobytes() == g.tobytes(), (c, st["scale"], g)
        assert st["scales"].tobytes() == per.tobytes(), (c, st["scales"], per)
    if mode == "global":
        assert _read(case, ops.segment_norms(case["flat"], case["plan"], mode=mode, threshold=thresholds[1]))["scale"] == 1.0
    else:
        st = _read(case, ops.segment_norms(case["flat"], case["plan"], mode=mode, threshold=thresholds[2]))
        assert st["scales"][2] == 1.0 and st["scales"][7] == 1.0 and st["scales"].min() < 1.0      # boundary and zero norm: 1
    from sketchformer_amd import _lib
    with pytest.raises(_lib.SkfError, match="threshold"):
        ops.segment_norms(case["flat"], case["plan"], mode=mode, threshold=0.0)


def test_segment_scale_equals_the_strided_views_times_their_scales(case):
    ops = case["ops"]
    c = float(np.median(case["per"]))
    stats = ops.segment_norms(case["flat"], case["plan"], mode="per_variable", threshold=c)
    E = len(ENTRIES)
    scales = stats[8 + E:8 + 2 * E]
    want = case["flat"].clone()
    for i, e in enumerate(ENTRIES):
        v = torch.as_strided(want, (e["rows"], e["cols"]), (e["row_stride"], 1), e["offset"])
        v.copy_(v * scales[i])
    got = case["flat"].clone()
    ops.segment_scale_(got, case["plan"], scales)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    gaps = torch.from_numpy(_gap_mask()).cuda()
    assert torch.isnan(got[gaps]).all() and not torch.isnan(got[~gaps]).any()
    assert not torch.equal(got.view(torch.int32), case["flat"].view(torch.int32))
    # with the skip word set nothing is written
    untouched = case["flat"].clone()
    ops.segment_scale_(untouched, case["plan"], scales, skip=torch.ones(1, dtype=torch.int32, device="cuda"))
    assert torch.equal(untouched.view(torch.int32), case["flat"].view(torch.int32))


def test_nonfinite_elements_are_counted_and_set_the_skip_flag(case):
    """Ordinary arithmetic on inf / NaN values: counted per element, wherever they sit."""
    ops = case["ops"]
    bad = case["flat"].clone()
    k = ENTRIES[4]
    bad[k["offset"] + 3 * k["row_stride"] + k["cols"] - 1] = float("inf")          # the last element of a strided row
    bad[BIG + R.CHUNK + 17] = float("-inf")                                         # inside the second chunk of the long entry
    bad[ENTRIES[1]["offset"] + 2] = float("nan")                                     # a scalar-tail element
    st = _read(case, ops.segment_norms(bad, case["plan"], mode="global", threshold=1.0, skip_nonfinite=True))
    assert st["nonfinite"] == 3 and st["skipped"]
    st = _read(case, ops.segment_norms(bad, case["plan"], mode="global", threshold=1.0, skip_nonfinite=False))
    assert st["nonfinite"] == 3 and not st["skipped"]
    st = _read(case, ops.segment_norms(case["flat"], case["plan"], skip_nonfinite=True))
    assert st["nonfinite"] == 0 and not st["skipped"]


def _sweep_operands(n, seed):
    rng = np.random.RandomState(seed)
    mk = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()      # noqa: E731
    return mk(rng.randn(n)), mk(rng.randn(n) * np.exp(rng.randn(n))), mk(0.1 * rng.randn(n)), mk(0.01 * rng.rand(n))


@pytest.mark.parametrize("n", [1, 5, 4 * 256 * 3 + 2])
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_clipped_sweeps_equal_the_plain_sweep_over_a_prescaled_gradient(case, n, optimizer):
    ops = case["ops"]
    st = ops.new_step_state("cuda", iterations=3000)
    ops.step_prologue(st)
    assert ops.read_step_state(st)["lr"] > 0
    w0, g, m0, v0 = _sweep_operands(n, n)
    s = torch.tensor([0.37], dtype=torch.float32, device="cuda")
    cv = float(g.abs().median())

    def plain(grad):
        w, m, v = w0.clone(), m0.clone(), v0.clone()
        if optimizer == "adam":
            ops.adam_step(w, grad, m, v, st)
        else:
            ops.sgd_momentum_step(w, grad, m, st)
        return w, m, v

    def clipped(**kw):
        w, m, v = w0.clone(), m0.clone(), v0.clone()
        if optimizer == "adam":
            ops.adam_step_clipped(w, g, m, v, st, **kw)
        else:
            ops.sgd_momentum_step_clipped(w, g, m, st, **kw)
        return w, m, v

    for kw, grad in ((dict(scale=s), g * s), (dict(clipvalue=cv), g.clamp(-cv, cv)), (dict(), g)):
        for got, want in zip(clipped(**kw), plain(grad)):
            assert torch.equal(got, want), (optimizer, n, sorted(kw))
    assert not torch.equal(clipped(scale=s)[0], plain(g)[0])
    assert ops.read_step_state(st)["iterations"] == 3000           # advance=False: the sweep does not close the step
    # the skip words {flag, total}: set -> nothing changes, iterations stay, the total counts; clear -> the step closes
    skip = torch.tensor([1, 4], dtype=torch.int32, device="cuda")
    for got, want in zip(clipped(scale=s, skip=skip, advance=True), (w0, m0, v0)):
        assert torch.equal(got, want)
    assert ops.read_step_state(st)["iterations"] == 3000 and skip.tolist() == [1, 5]
    skip[0] = 0
    for got, want in zip(clipped(scale=s, skip=skip, advance=True), plain(g * s)):
        assert torch.equal(got, want)
    assert ops.read_step_state(st)["iterations"] == 3001 and skip.tolist() == [0, 5]
