"""Device arc-length resampling against the host restatement of tests/resample_reference.py (tests/test_resample_cpu.py asserts
the restatement's facts on the CPU).  Everything is equality on bit patterns - rows, offsets, shapes - there are no tolerances
but the two of the alignment test, which the issue states."""
import numpy as np
import pytest
import torch

import resample_reference as rr
import simplify_reference as ref
from sketchformer_amd import _lib, align, ops, simplify

pytestmark = pytest.mark.gpu

DEV = "cuda"
ABOVE_THE_SCAN_BLOCK = 2 * ref.OFFSETS_SCAN_BLOCK + 5
STROKE_COUNTS = (1, 63, 64, 65, ABOVE_THE_SCAN_BLOCK)
LONG = np.array([(0, 0), (3000, 4000), (6000, 0), (6000, 1.5)], np.float32)      # 10001.5 units: several thousand rows at spacing 1


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # (a copy: the shared references are read-only)


def _resample(lines, spacing):
    xy, offsets = ref.pack_lines(lines)
    out_xy, out_offsets = ops.polyline_resample(_dev(xy), _dev(offsets), spacing)
    assert out_xy.dtype == torch.float32 and out_xy.dim() == 2 and out_xy.shape[1] == 2 and out_xy.is_contiguous()
    assert out_offsets.dtype == torch.int64 and tuple(out_offsets.shape) == (len(lines) + 1,)
    return out_xy.cpu().numpy(), out_offsets.cpu().numpy()


def _check(lines, spacing, want=None):
    got_xy, got_offsets = _resample(lines, spacing)
    want_xy, want_offsets = rr.pack(rr.resample_all(lines, spacing) if want is None else want)
    assert np.array_equal(got_offsets, want_offsets)
    assert rr.same_bits(got_xy, want_xy)
    return got_xy, got_offsets


@pytest.fixture(scope="module")
def pools():
    pool = {"int": ref.int_pool(), "float": ref.float_pool()}
    assert {0, 1, 2, 3, 63, 64, 65, 130, ref.LDS_POINTS - 1, ref.LDS_POINTS + 1, ref.LDS_POINTS + 5} <= {len(l) for l in pool["float"]}
    return pool


@pytest.fixture(scope="module")
def short():
    lines = ref.short_strokes(ABOVE_THE_SCAN_BLOCK)
    return lines, rr.resample_all(lines, 1.0)


# ---------------------------------------------------------------- ops.polyline_resample
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("spacing", [1.0, 2.5, 1e6])
def test_resample_matches_the_restatement(pools, kind, spacing):
    lines = pools[kind]
    _, offsets = _check(lines, spacing)
    if spacing == 1e6:                                                       # larger than every total: the two ends, or one row
        rows = np.diff(offsets)
        assert set(rows.tolist()) <= {0, 1, 2} and (rows == 2).sum() > 10


def test_resample_on_the_named_fixtures():
    got, offsets = _check([rr.LINE_0_10, rr.PYTHAGORAS, rr.PYTHAGORAS[:1], np.repeat(rr.PYTHAGORAS[1:2], 4, axis=0)], 1.0)
    assert offsets.tolist() == [0, 11, 32, 33, 34]
    assert got[:11].tolist() == [[float(k), 0.0] for k in range(11)]
    assert rr.same_bits(got[11:32:5], rr.PYTHAGORAS) and got[12].tolist() == [np.float32(0.6), np.float32(0.8)]


def test_resample_row_counts_around_a_wave_and_far_above_it():
    lines = [np.array([(0, 0), (63, 0)], np.float32), np.array([(1, 1), (1, 65)], np.float32), LONG, np.array([(0, 0), (62.5, 0)], np.float32)]
    _, offsets = _check(lines, 1.0)
    assert np.diff(offsets).tolist() == [64, 65, 10003, 64]
    _, offsets = _check(lines, 2.0 ** -3)                                    # 8 rows a unit: 80 013 rows on one polyline
    assert np.diff(offsets).tolist() == [505, 513, 80013, 501]


@pytest.mark.parametrize("S", STROKE_COUNTS)
def test_resample_stroke_counts(short, S):
    lines, want = short
    _check(lines[:S], 1.0, want=want[:S])


def test_resample_reads_rows_of_any_stride_and_leaves_its_inputs_alone(pools):
    lines = pools["int"][:30]
    xy, offsets = ref.pack_lines(lines)
    wide = torch.full((len(xy), 5), float("nan"), device=DEV)
    wide[:, 1:3] = _dev(xy)
    before, off_d = wide.clone(), _dev(offsets)
    view = wide[:, 1:3]                                                      # ldp = 5
    first = ops.polyline_resample(view, off_d, 1.0)
    again = ops.polyline_resample(view, off_d, 1.0)
    want_xy, want_offsets = rr.pack(rr.resample_all(lines, 1.0))
    assert rr.same_bits(first[0].cpu().numpy(), want_xy) and np.array_equal(first[1].cpu().numpy(), want_offsets)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    assert torch.equal(wide.view(torch.int32), before.view(torch.int32)) and np.array_equal(off_d.cpu().numpy(), offsets)
    dense = ops.polyline_resample_n(view, off_d, 33)
    assert rr.same_bits(dense.cpu().numpy(), np.stack([rr.resample_n(l, 33) for l in lines]))
    one = torch.tensor([[3.0, 4.0]], device=DEV)
    for bad in (one.expand(2, 2), torch.arange(3.0, device=DEV).as_strided((2, 2), (1, 1))):      # row strides 0 and 1
        with pytest.raises(ValueError, match="overlap"):
            ops.polyline_resample(bad, torch.tensor([0, 2], device=DEV), 1.0)


def test_offsets_outside_the_rows_are_clamped():
    """Negative, past the end, descending: the clamp to [0, P] defines the answer - rows 0 .. 5, rows 6 .. 9, nothing."""
    line = ref.smooth_int_stroke(np.random.RandomState(5), 10)
    xy_d = _dev(line)
    offsets = torch.tensor([-5, 6, 12, 8], dtype=torch.int64, device=DEV)
    want_xy, want_offsets = rr.pack([rr.resample(line[:6], 1.0), rr.resample(line[6:], 1.0), np.zeros((0, 2), np.float32)])
    got_xy, got_offsets = ops.polyline_resample(xy_d, offsets, 1.0)
    assert np.array_equal(got_offsets.cpu().numpy(), want_offsets) and rr.same_bits(got_xy.cpu().numpy(), want_xy)
    dense = ops.polyline_resample_n(xy_d, offsets, 9).cpu().numpy()
    assert rr.same_bits(dense, np.stack([rr.resample_n(line[:6], 9), rr.resample_n(line[6:], 9), np.zeros((9, 2), np.float32)]))
    assert rr.same_bits(xy_d.cpu().numpy(), line)


# ---------------------------------------------------------------- the C ABI
def _abi():
    lib = _lib.load()
    line = np.concatenate([rr.PYTHAGORAS, rr.LINE_0_10])
    st = {"lib": lib, "xy": _dev(line), "offsets": _dev(np.array([0, 5, 7], np.int64)),
          "out_offsets": torch.full((3,), -7, dtype=torch.int64, device=DEV),
          "out": torch.full((40, 2), -7.0, dtype=torch.float32, device=DEV)}
    st["ws_bytes"] = lib.skf_polyline_resample_workspace_bytes(7, 2)
    assert st["ws_bytes"] > 0
    st["ws"] = torch.zeros(st["ws_bytes"] + 64, dtype=torch.uint8, device=DEV)
    st["want"] = np.concatenate([rr.resample(rr.PYTHAGORAS, 1.0), rr.resample(rr.LINE_0_10, 1.0)])
    return st


def test_out_rows_is_a_capacity():
    st = _abi()
    lib, p = st["lib"], {k: st[k].data_ptr() for k in ("xy", "offsets", "out_offsets", "out", "ws")}
    assert lib.skf_polyline_resample_count(p["xy"], 2, 7, p["offsets"], 2, 1.0, p["out_offsets"], p["ws"], st["ws_bytes"], None) == 0
    torch.cuda.synchronize()
    assert st["out_offsets"].tolist() == [0, 21, 32] and (st["out"] == -7).all()
    for cap in (25, 21, 1):                                                  # inside the second polyline, between the two, one row
        st["out"].fill_(-7.0)
        assert lib.skf_polyline_resample_emit(p["xy"], 2, 7, p["offsets"], 2, 1.0, p["out_offsets"], p["out"], cap, p["ws"],
                                              st["ws_bytes"], None) == 0
        torch.cuda.synchronize()
        got = st["out"].cpu().numpy()
        assert rr.same_bits(got[:cap], st["want"][:cap]) and (got[cap:] == -7).all(), cap
    st["out"].fill_(-7.0)
    assert lib.skf_polyline_resample_emit(p["xy"], 2, 7, p["offsets"], 2, 1.0, p["out_offsets"], p["out"], 40, p["ws"], st["ws_bytes"], None) == 0
    torch.cuda.synchronize()
    got = st["out"].cpu().numpy()
    assert rr.same_bits(got[:32], st["want"]) and (got[32:] == -7).all()     # rows no polyline owns stay as they were


def test_argument_limits_are_refused_with_their_message():
    st = _abi()
    lib = st["lib"]
    base = {k: st[k].data_ptr() for k in ("xy", "offsets", "out_offsets", "out", "ws")}

    def count(P=7, S=2, ldp=2, spacing=1.0, ws_bytes=st["ws_bytes"], shift=None, **_):
        p = dict(base)
        if shift:
            p[shift[0]] += shift[1]
        return lib.skf_polyline_resample_count(p["xy"], ldp, P, p["offsets"], S, spacing, p["out_offsets"], p["ws"], ws_bytes, None)

    def emit(P=7, S=2, ldp=2, spacing=1.0, out_rows=40, ws_bytes=st["ws_bytes"], shift=None, **_):
        p = dict(base)
        if shift:
            p[shift[0]] += shift[1]
        return lib.skf_polyline_resample_emit(p["xy"], ldp, P, p["offsets"], S, spacing, p["out_offsets"], p["out"], out_rows, p["ws"],
                                              ws_bytes, None)

    def dense(P=7, S=2, ldp=2, n_out=8, ws_bytes=st["ws_bytes"], shift=None, **_):
        p = dict(base)
        if shift:
            p[shift[0]] += shift[1]
        return lib.skf_polyline_resample_n(p["xy"], ldp, P, p["offsets"], S, n_out, p["out"], p["ws"], ws_bytes, None)

    shared = [(dict(S=0), "S must be at least 1"), (dict(S=-1), "S must be at least 1"), (dict(P=0), "P must be in"),
              (dict(P=1 << 31), "P must be in"), (dict(ldp=1), "ldp must be at least 2"), (dict(ws_bytes=8), "workspace too small"),
              (dict(ws_bytes=st["ws_bytes"] - 1), "workspace too small"), (dict(shift=("xy", 2)), "aligned"),
              (dict(shift=("offsets", 4)), "aligned"), (dict(shift=("ws", 8)), "aligned")]
    spacings = [(dict(spacing=s), "spacing must be finite") for s in (0.0, -1.0, 2.0 ** -17, float("nan"), float("inf"), 1e14)]
    cases = [(count, shared + spacings + [(dict(shift=("out_offsets", 4)), "8-byte aligned")]),
             (emit, shared + spacings + [(dict(shift=("out_offsets", 4)), "8-byte aligned"), (dict(shift=("out", 4)), "8-byte aligned"),
                                         (dict(out_rows=0), "out_rows must be in"), (dict(out_rows=-1), "out_rows must be in"),
                                         (dict(out_rows=1 << 31), "out_rows must be in")]),
             (dense, shared + [(dict(shift=("out", 4)), "8-byte aligned"), (dict(n_out=1), "n_out must be in"), (dict(n_out=0), "n_out must be in"),
                               (dict(n_out=65537), "n_out must be in")])]
    for fn, bads in cases:
        for bad, text in bads:
            assert fn(**bad) == -1, (fn.__name__, bad)
            message = lib.skf_last_error().decode()
            assert text in message and ("skf_polyline_resample_" + {"dense": "n"}.get(fn.__name__, fn.__name__)) in message, (bad, message)
    torch.cuda.synchronize()
    assert (st["out"] == -7).all() and (st["out_offsets"] == -7).all()       # nothing was launched
    assert count() == 0 and emit() == 0 and count(spacing=2.0 ** -16) == 0 and dense(n_out=2) == 0 and dense(n_out=20) == 0
    torch.cuda.synchronize()
    # the wrappers refuse on the host
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spacing"):
            ops.polyline_resample(st["xy"], st["offsets"], bad)
    for bad in (1, 65537):
        with pytest.raises(ValueError, match="n_out"):
            ops.polyline_resample_n(st["xy"], st["offsets"], bad)
    with pytest.raises(TypeError):
        ops.polyline_resample(st["xy"].double(), st["offsets"], 1.0)
    with pytest.raises(TypeError):
        ops.polyline_resample_n(st["xy"], st["offsets"].to(torch.int32), 8)


# ---------------------------------------------------------------- ops.polyline_resample_n
@pytest.mark.parametrize("n_out", [2, 33, 64, 65, 256])
def test_resample_n_matches_the_restatement(pools, n_out):
    lines = pools["int"] + pools["float"] + [LONG, rr.PYTHAGORAS, np.repeat(rr.PYTHAGORAS[:1], 3, axis=0)]
    xy, offsets = ref.pack_lines(lines)
    xy_d, off_d = _dev(xy), _dev(offsets)
    got = ops.polyline_resample_n(xy_d, off_d, n_out)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(lines), n_out, 2) and got.is_contiguous()
    want = np.stack([rr.resample_n(l, n_out) for l in lines])
    assert rr.same_bits(got.cpu().numpy(), want)
    empties = [i for i, l in enumerate(lines) if len(l) == 0]
    assert empties and not want[empties].any()                               # an empty polyline: n_out rows (0, 0)
    assert torch.equal(got.view(torch.int32), ops.polyline_resample_n(xy_d, off_d, n_out).view(torch.int32))


# ---------------------------------------------------------------- through the Python layers
def test_resample_lines(pools):
    lines = pools["float"][:9] + pools["int"][13:30]
    got = simplify.resample_lines([l.astype(np.float64) for l in lines], spacing=2.5)
    tiny = simplify.resample_lines(lines, spacing=2.5, row_budget=50)
    for g, t, l in zip(got, tiny, lines):
        want = rr.resample(l, 2.5)
        assert g.dtype == np.float32 and rr.same_bits(g, want) and rr.same_bits(t, want)
    got = simplify.resample_lines(lines, n_points=16, row_budget=40)         # two polylines a call
    for g, l in zip(got, lines):
        assert rr.same_bits(g, rr.resample_n(l, 16))


@pytest.mark.parametrize("row_budget", [None, 300])
def test_simplify_lines_with_resampling(pools, monkeypatch, row_budget):
    lines = pools["int"][:30] + pools["float"][:8] + [rr.PYTHAGORAS]
    calls = []
    real = ops.polyline_resample
    monkeypatch.setattr(ops, "polyline_resample", lambda *a: calls.append(int(a[1].shape[0]) - 1) or real(*a))
    got = simplify.simplify_lines(lines, 2.0, resample_spacing=1.0, row_budget=row_budget)
    resampled = rr.resample_all(lines, 1.0)
    assert sum(calls) <= len(lines)
    if row_budget is None:
        assert len(calls) == 1
    else:                                                                    # the batch was cut, and no call went over the budget
        assert len(calls) > 3 and max(len(r) for r in resampled) > row_budget
    for g, r in zip(got, resampled):
        assert g.dtype == np.float32 and rr.same_bits(g, r[ref.rdp_mask(r, 2.0) != 0])
    # without the keyword: today's result, in the caller's dtype
    plain = simplify.simplify_lines([l.astype(np.float64) for l in lines[:20]], 2.0)
    for g, l in zip(plain, lines):
        assert g.dtype == np.float64 and np.array_equal(g, l[ref.rdp_mask(l, 2.0) != 0])


def test_dtw_after_resampling_does_not_see_the_vertex_density():
    def stroke3(points):
        s = np.zeros((len(points), 3), np.float32)
        s[0, :2], s[1:, :2] = points[0], points[1:] - points[:-1]
        s[-1, 2] = 1
        return s

    a, b = rr.PYTHAGORAS, rr.split_at_midpoints(rr.PYTHAGORAS)
    assert len(b) == 9 and rr.same_bits(b[::2], a) and b[1].tolist() == [1.5, 2.0]
    n = 64
    with_resampling = float(align.sketch_dtw([stroke3(a)], [stroke3(b)], normalize=False, resample=n)[0])
    without = float(align.sketch_dtw([stroke3(a)], [stroke3(b)], normalize=False)[0])
    print("dtw with resampling %.3e, without %.3e" % (with_resampling, without))
    assert 0.0 <= with_resampling < 1e-4 * n
    assert without >= 10.0 - 1e-3                                            # four midpoints, each 2.5 from the nearest vertex
    # normalised: n + n steps; an empty sketch is n copies of (0, 0)
    d = align.sketch_dtw([stroke3(a), np.zeros((0, 3), np.float32)], [stroke3(b), np.zeros((0, 3), np.float32)], resample=n)
    assert d.dtype == torch.float64 and float(d[0]) == pytest.approx(with_resampling / (2 * n)) and float(d[1]) == 0.0
    with pytest.raises(ValueError, match="resample"):
        align.sketch_dtw([stroke3(a)], [stroke3(b)], resample=1)
    with pytest.raises(ValueError, match="resample"):
        align.sketch_dtw([stroke3(a)], [stroke3(b)], resample=513)


def test_sequence_retrieval_with_resample_points(tmp_path):
    import types
    import align_reference as aref
    from sketchformer_amd import dataloaders, experiments
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=4,n_samples=64"), None)
    model = types.SimpleNamespace(dataset=dataset)                           # the experiment uses model.dataset only
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    exp = Exp(Exp.parse_hparams("distance=dtw,n_queries=6,n_gallery=20,top_k=5,gallery_block=12,resample_points=16"), "s0", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    tok = dataset.tokenizer
    gx = dataset.get_all_data_from("test")[0][out["gallery_rows"]]
    qx = dataset.get_all_data_from("valid")[0][out["query_rows"]]

    def path(row):
        return rr.resample_n(aref.decoded_points(row, tok), 16)
    D = np.array([[aref.dtw_ref(path(q), path(g)) for g in gx] for q in qx], np.float32)
    want = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert np.array_equal(out["indices"], want)
    assert rr.same_bits(out["distances"], np.take_along_axis(D, want, axis=1))
    plain = np.array([[aref.dtw_ref(aref.decoded_points(q, tok), aref.decoded_points(g, tok)) for g in gx] for q in qx], np.float32)
    assert not np.array_equal(D, plain)                                      # the hparam reached the distance
