"""Device stroke edits against the host restatement of tests/strokes_reference.py (tests/test_strokes_cpu.py asserts the
restatement's own facts on the CPU).  Everything is equality on bit patterns - rows, offsets, tables - through the C ABI; there
are no tolerances but the cosine bound of the experiment test, which is stated there."""
import numpy as np
import pytest
import torch

import align_reference as ar
import preprocess_reference as pref
import strokes_reference as st
from sketchformer_amd import _lib, ops, strokes
from sketchformer_amd.utils.tokenizer import GridTokenizer

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = -7.0


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@pytest.fixture(scope="module")
def batch():
    b = st.table_batch()
    lens = sorted({hi - lo + 1 for s in b for lo, hi in st.stroke_ranges(s)})
    assert {1, 2, 63, 64, 65, 130} <= set(lens) and max(len(s) for s in b) > 512
    assert len(b[0]) == 0 and len(b[-1]) == 0 and any(len(s) == 0 for s in b[1:-1])
    return b


@pytest.fixture(scope="module")
def want_table(batch):
    return st.stroke_table(batch)


@pytest.fixture(scope="module")
def cases(batch):
    src, lists = st.edit_cases(batch)
    want = st.edit(batch, src, lists)
    assert {0, 1, 64, 65, 129} <= {len(l) for l in lists} and len(src) > len(batch)
    assert any(a > b for a, b in zip(src, src[1:]))                            # src is not monotonic
    return src, lists, want


def _table(batch):
    flat, offsets = st.pack(batch)
    return ops.stroke_table(_dev(flat), _dev(offsets))


def _same_table(got, want):
    ss, sr_, se = (t.cpu().numpy() for t in got)
    return np.array_equal(ss, want[0]) and np.array_equal(sr_, want[1]) and st.same_bits(se, want[2])


# ---------------------------------------------------------------- the table
def test_stroke_table_matches_the_restatement(batch, want_table):
    got = _table(batch)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    assert tuple(got[2].shape) == (int(want_table[0][-1]), 4)
    assert _same_table(got, want_table)
    assert _same_table(_table(batch), want_table)                              # two calls agree
    counts = np.diff(want_table[0])
    assert counts.tolist()[:5] == [0, 6, 1, 65, 2] and counts[-2] == 1         # pen 2 ends no stroke
    assert np.array_equal(strokes.stroke_counts(batch), counts)
    flat, offsets = st.pack(batch)
    assert np.array_equal(strokes.stroke_counts((_dev(flat), _dev(offsets))), counts)


def test_stroke_table_of_single_sketches(batch, want_table):
    """N = 1 and a sketch's table does not depend on the rest of the batch."""
    for i in (1, 3, 6, 7):
        assert _same_table(_table([batch[i]]), st.stroke_table([batch[i]])), i


def test_table_offsets_outside_the_rows_are_clamped():
    """Negative, past the end, descending: the clamp to [0, P] defines the answer - rows 0 .. 5, rows 6 .. 9, nothing."""
    s = st.int_sketch(np.random.RandomState(5), [3, 4, 3])
    offsets = torch.tensor([-5, 6, 12, 8], dtype=torch.int64, device=DEV)
    got = ops.stroke_table(_dev(s), offsets)
    want = st.stroke_table([s[:6], s[6:], s[:0]])
    assert _same_table(got, want)


# ---------------------------------------------------------------- the edit
def _edit(batch, src, lists, table=None):
    flat, offsets = st.pack(batch)
    sel, sel_offsets = st.pack_lists(lists)
    out = ops.stroke_edit(_dev(flat), _dev(offsets), _dev(np.asarray(src, np.int32)), _dev(sel_offsets), _dev(sel), table=table)
    assert out[0].dtype == torch.float32 and out[0].dim() == 2 and out[0].shape[1] == 3 and out[0].is_contiguous()
    assert out[1].dtype == torch.int64 and tuple(out[1].shape) == (len(src) + 1,)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def test_stroke_edit_matches_the_restatement(batch, cases):
    src, lists, want = cases
    want_flat, want_offsets = st.pack(want)
    got_flat, got_offsets = _edit(batch, src, lists)
    assert np.array_equal(got_offsets, want_offsets)
    assert st.same_bits(got_flat, want_flat), np.argwhere(got_flat.view(np.int32) != want_flat.view(np.int32))[:5]
    again = _edit(batch, src, lists, table=_table(batch))                      # two calls agree, with a table handed in
    assert st.same_bits(again[0], got_flat) and np.array_equal(again[1], got_offsets)
    rows = np.diff(want_offsets)
    assert rows[0] == 0 and rows[7] == 0 and rows[8] == 0 and rows[9] == 0     # an empty list, src = -1, src = N, an empty source
    assert (got_flat.view(np.int32) == np.float32(-0.0).view(np.int32)).any()  # a sign flip made a -0


def test_stroke_edit_fewer_outputs_than_sketches_and_an_empty_result(batch):
    src, lists = [7, 1], [[~1], [3, 3]]                                         # M < N
    got_flat, got_offsets = _edit(batch, src, lists)
    want_flat, want_offsets = st.pack(st.edit(batch, src, lists))
    assert np.array_equal(got_offsets, want_offsets) and st.same_bits(got_flat, want_flat)
    for src, lists in (([0, -1, 5], [[0], [0, 1], [~0]]), ([1, 2], [[], []]), ([1], [[6, ~6]])):       # P' = 0
        got_flat, got_offsets = _edit(batch, src, lists)
        assert got_flat.shape == (0, 3) and got_offsets.tolist() == [0] * (len(src) + 1)


def test_strokes_module_matches_the_restatement(batch):
    """The list builders through the device, on lists of arrays and on a device pair."""
    live = [s for s in batch if len(s)]
    counts = [len(st.stroke_ranges(s)) for s in live]
    orders = [np.random.RandomState(9).permutation(c) for c in counts]
    rng = np.random.RandomState(4)
    drawn = [rng.permutation(c) for c in counts]
    flat, offsets = st.pack(live)
    pair = (_dev(flat), _dev(offsets))
    checks = [(strokes.permute_strokes, dict(orders=orders), orders),
              (strokes.permute_strokes, dict(seed=4), drawn),
              (strokes.reverse_strokes, dict(), [~np.arange(c) for c in counts]),
              (strokes.reverse_strokes, dict(order=True), [~np.arange(c)[::-1] for c in counts]),
              (strokes.reverse_strokes, dict(direction=False, order=True), [np.arange(c)[::-1] for c in counts]),
              (strokes.keep_first_strokes, dict(k=2), [np.arange(min(c, 2)) for c in counts])]
    for fn, kw, lists in checks:
        want = st.edit(live, range(len(live)), lists)
        got = fn(live, **kw)
        assert len(got) == len(want) and all(st.same_bits(g, w) for g, w in zip(got, want)), (fn.__name__, kw)
        got_flat, got_offsets = fn(pair, **kw)
        want_flat, want_offsets = st.pack(want)
        assert st.same_bits(got_flat.cpu().numpy(), want_flat) and np.array_equal(got_offsets.cpu().numpy(), want_offsets)
    with pytest.raises(IndexError):
        strokes.leave_one_stroke_out(batch)                                    # an empty sketch cannot be encoded


# ---------------------------------------------------------------- the C ABI: capacity, canaries, limits
def test_out_rows_is_a_capacity(batch, want_table, cases):
    src, lists, want = cases
    want_flat, want_offsets = st.pack(want)
    rows = len(want_flat)
    lib = _lib.load()
    flat, offsets = st.pack(batch)
    sel, sel_offsets = st.pack_lists(lists)
    P, N, M, Q, T = len(flat), len(batch), len(src), len(sel), len(want_table[1]) - 1
    t = {"flat": _dev(flat), "ss": _dev(want_table[0]), "sr": _dev(want_table[1]), "se": _dev(want_table[2]),
         "src": _dev(np.asarray(src, np.int32)), "so": _dev(sel_offsets), "sel": _dev(sel),
         "oo": torch.full((M + 1,), -7, dtype=torch.int64, device=DEV),
         "out": torch.full((rows + 50, 3), CANARY, dtype=torch.float32, device=DEV)}
    nbytes = lib.skf_stroke_edit_workspace_bytes(P, N, M, Q)
    assert nbytes > 0
    t["ws"] = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    p = {k: v.data_ptr() for k, v in t.items()}
    assert lib.skf_stroke_edit_count(P, p["ss"], N, p["sr"], T, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"], p["ws"], nbytes, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t["oo"].cpu().numpy(), want_offsets) and (t["out"] == CANARY).all()

    def emit(cap):
        t["out"].fill_(CANARY)
        assert lib.skf_stroke_edit_emit(p["flat"], P, p["ss"], N, p["sr"], p["se"], T, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"],
                                        p["out"], cap, p["ws"], nbytes, None) == 0
        torch.cuda.synchronize()
        return t["out"].cpu().numpy()
    got = emit(rows + 50)
    assert st.same_bits(got[:rows], want_flat) and (got[rows:] == CANARY).all()          # the canary rows stay untouched
    inside = int(want_offsets[5]) + 70                                         # inside a stroke, inside a sketch
    for cap in (inside, int(want_offsets[3]), 1):
        got = emit(cap)
        assert st.same_bits(got[:cap], want_flat[:cap]) and (got[cap:] == CANARY).all(), cap
    again = emit(rows)
    assert st.same_bits(again[:rows], want_flat)
    # limits
    assert lib.skf_stroke_edit_count(P, p["ss"], N, p["sr"], T, p["src"], p["so"], M, p["sel"], Q, 1, p["oo"], p["ws"], nbytes, None) != 0
    assert b"flag" in lib.skf_last_error()
    assert lib.skf_stroke_edit_count(P, p["ss"], N, p["sr"], T, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"], p["ws"] + 8, nbytes, None) != 0
    assert lib.skf_stroke_edit_count(P, p["ss"], N, p["sr"], P + 1, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"], p["ws"], nbytes, None) != 0
    assert lib.skf_stroke_edit_count(P, p["ss"], N, p["sr"], T, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"], p["ws"], nbytes - 1, None) != 0
    assert lib.skf_stroke_edit_emit(p["flat"], P, p["ss"], N, p["sr"], p["se"], T, p["src"], p["so"], M, p["sel"], Q, 0, p["oo"],
                                    p["out"], 0, p["ws"], nbytes, None) != 0


def test_stroke_edit_clamps_a_table_and_lists_that_lie(batch, want_table):
    """A sketch_strokes entry past T through ops; sel_offsets below 0 and past Q through the C ABI (ops refuses them): what the
    clamps leave is what comes out, and the canary rows stay."""
    flat, offsets = st.pack(batch)
    want = st.edit(batch, [1], [[0, 1]])[0]
    table = [_dev(want_table[0]), _dev(want_table[1]), _dev(want_table[2])]
    table[0][-1] += 1000                                                        # the last sketch owns strokes past T: clamped to T
    src = _dev(np.array([1, len(batch) - 1], np.int32))
    sel = _dev(np.array([0, 1, 2], np.int32))
    good = torch.tensor([0, 2, 3], dtype=torch.int64, device=DEV)
    got_flat, got_offsets = ops.stroke_edit(_dev(flat), _dev(offsets), src, good, sel, table=tuple(table))
    assert got_offsets.tolist() == [0, len(want), len(want)] and st.same_bits(got_flat.cpu().numpy(), want)
    for bad in ([-4, 2, 3], [0, 2, 99], [0, 3, 2], [1, 2, 3]):
        with pytest.raises(ValueError, match="sel_offsets"):
            ops.stroke_edit(_dev(flat), _dev(offsets), src, torch.tensor(bad, dtype=torch.int64, device=DEV), sel, table=tuple(table))
    lib = _lib.load()
    P, N, M, Q, T = len(flat), len(batch), 2, 3, len(want_table[1]) - 1
    lying = torch.tensor([-4, 2, 99], dtype=torch.int64, device=DEV)           # the lists [0, 2) and [2, 3)
    flat_d, oo = _dev(flat), torch.full((M + 1,), -7, dtype=torch.int64, device=DEV)
    out = torch.full((len(want) + 9, 3), CANARY, dtype=torch.float32, device=DEV)
    nbytes = lib.skf_stroke_edit_workspace_bytes(P, N, M, Q)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    args = (table[0].data_ptr(), N, table[1].data_ptr())
    assert lib.skf_stroke_edit_count(P, *args, T, src.data_ptr(), lying.data_ptr(), M, sel.data_ptr(), Q, 0, oo.data_ptr(), ws.data_ptr(),
                                     nbytes, None) == 0
    assert lib.skf_stroke_edit_emit(flat_d.data_ptr(), P, *args, table[2].data_ptr(), T, src.data_ptr(), lying.data_ptr(), M, sel.data_ptr(),
                                    Q, 0, oo.data_ptr(), out.data_ptr(), out.shape[0], ws.data_ptr(), nbytes, None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert oo.tolist() == [0, len(want), len(want)] and st.same_bits(got[:len(want)], want) and (got[len(want):] == CANARY).all()


# ---------------------------------------------------------------- ink is preserved, order is not
def _points(flat, offsets):
    """(flat, offsets) device tensors -> what ops.sketch_points returns for them"""
    off = offsets.cpu().numpy()
    n = np.diff(off).astype(np.int32)
    dense = torch.zeros(len(n), int(n.max()), 3, dtype=torch.float32, device=DEV)
    for i in range(len(n)):
        dense[i, :n[i]] = flat[off[i]:off[i + 1]]
    return ops.sketch_points(dense, 'stroke3', lengths=_dev(n))


def test_edits_preserve_the_ink_and_change_the_order():
    sketches, orders = st.ink_fixture()
    flat, offsets = st.pack(sketches)
    pair = (_dev(flat), _dev(offsets))
    control = strokes.edit(pair, np.arange(len(sketches)), strokes.identity_lists(strokes.stroke_counts(sketches)))
    assert st.same_bits(control[0].cpu().numpy(), flat)                        # integer data: the identity returns the input
    xa, pa, na, _ = _points(*control)
    kinds = {"permuted": strokes.permute_strokes(pair, orders=orders), "direction": strokes.reverse_strokes(pair),
             "time": strokes.reverse_strokes(pair, order=True)}
    for name, variant in kinds.items():
        xb, pb, nb, _ = _points(*variant)
        parts = ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=1).cpu().numpy()
        assert parts.shape == (len(sketches), 4) and (parts == 0).all(), (name, parts)
        dtw = ops.dtw_distance(xa, na, xb, nb).cpu().numpy()
        want_v = st.edit(sketches, range(len(sketches)), {"permuted": orders,
                                                          "direction": strokes.reverse_lists(strokes.stroke_counts(sketches)),
                                                          "time": strokes.reverse_lists(strokes.stroke_counts(sketches), order=True)}[name])
        want = np.array([ar.dtw_ref(np.cumsum(s[:, :2], axis=0, dtype=np.float32), np.cumsum(v[:, :2], axis=0, dtype=np.float32))
                         for s, v in zip(sketches, want_v)], np.float32)
        assert (dtw > 0).all() and st.same_bits(dtw, want), (name, dtw, want)


# ---------------------------------------------------------------- variants go straight into the encoder
@pytest.mark.parametrize("mode", ["grid", "stroke5"])
def test_leave_one_stroke_out_encodes_like_the_host_loader(batch, mode):
    live = [s for s in batch if len(s)]
    flat, offsets = st.pack(live)
    (vflat, voffsets), owner, dropped = strokes.leave_one_stroke_out((_dev(flat), _dev(offsets)))
    lists, want_owner, want_dropped = strokes.leave_one_out_lists([len(st.stroke_ranges(s)) for s in live])
    assert np.array_equal(owner, want_owner) and np.array_equal(dropped, want_dropped) and len(owner) > 70
    restated = st.edit(live, want_owner, lists)
    L = 96
    if mode == "grid":
        tok = GridTokenizer(resolution=100)
        loader = pref.host_loader(tokenizer=tok, max_seq_len=L, token_type="grid")
        got = ops.sketch_encode(vflat, voffsets, 'grid', L, resolution=100, clamp=False).cpu().numpy()
    else:
        loader = pref.host_loader(max_seq_len=L, use_continuous_data=True)
        got = ops.sketch_encode(vflat, voffsets, 'stroke5', L, clamp=False).cpu().numpy().astype(np.float64)
    want = loader.preprocess_per_sketch_from([np.array(s, dtype=np.float32) for s in restated])
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------- the experiment
def test_stroke_sensitivity_experiment(tmp_path):
    """stroke3-synthetic with the grid tokenizer its ids belong to (resolution 8: 64 cells + PAD, SEP, SOS, EOS = 68 ids, and cell
    centres on multiples of 1/8, so every position and every jump below is exact in fp32) and a freshly initialised small model."""
    from sketchformer_amd import dataloaders, experiments, models
    R, L, n, n_perm = 8, 24, 8, 2
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=%d,vocab_size=%d,n_classes=7,n_samples=64" % (L, R * R + 4)), None)
    tok = GridTokenizer(resolution=R)
    assert (tok.SEP, tok.SOS, tok.EOS) == (dataset.tokenizer.SEP, dataset.tokenizer.SOS, dataset.tokenizer.EOS)
    dataset.tokenizer = tok
    model = Model(Model.parse_hparams(base="batch_size=8,num_epochs=1,log_every=4",
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "ss")
    Exp = experiments.get_experiment_by_name("stroke-sensitivity")
    exp = Exp(Exp.parse_hparams("n_sketches=%d,n_permutations=%d,max_variants_per_batch=13" % (n, n_perm)), "s0", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    x = out["inputs"]
    decoded = [np.asarray(tok.decode_single(r), np.float32).reshape(-1, 3) for r in x]
    counts = np.array([len(st.stroke_ranges(s)) for s in decoded])
    V = int(counts[counts >= 2].sum())
    assert V > 0 and np.array_equal(out["stroke_count"], counts)
    E = 64                                                                     # (the version-1 bottleneck is d_model wide)
    for key, shape in (("inputs", (n, L)), ("labels", (n,)), ("control_input", (n, L)), ("control_embedding", (n, E)),
                       ("control_p_true", (n,)), ("control_class", (n,)),
                       ("permutation_cosine", (n_perm, n)), ("permutation_p_true", (n_perm, n)), ("permutation_class_changed", (n_perm, n)),
                       ("permutation_dtw", (n_perm, n)), ("permutation_chamfer", (n_perm, n)),
                       ("direction_cosine", (n,)), ("direction_p_true", (n,)), ("direction_class_changed", (n,)), ("direction_dtw", (n,)),
                       ("direction_chamfer", (n,)), ("time_cosine", (n,)), ("time_p_true", (n,)), ("time_class_changed", (n,)),
                       ("time_dtw", (n,)), ("time_chamfer", (n,)),
                       ("loo_owner", (V,)), ("loo_dropped", (V,)), ("loo_share", (V,)), ("loo_importance", (V,)), ("loo_p_true", (V,)),
                       ("loo_cosine", (V,)), ("loo_dtw", (V,)), ("loo_chamfer", (V,)),
                       ("kind", (3,)), ("cosine", (3,)), ("p_true", (3,)), ("p_true_drop", (3,)), ("class_changed", (3,)), ("dtw", (3,)),
                       ("chamfer", (3,)), ("rank", (5,)), ("rank_importance", (5,)), ("rank_count", (5,)), ("share_edges", (5,)),
                       ("share_importance", (4,)), ("share_count", (4,))):
        assert out[key].shape == shape, (key, out[key].shape)
    # the control is the host loader's encoding of the decoded sketches
    loader = pref.host_loader(tokenizer=tok, max_seq_len=L, token_type="grid")
    want = loader.preprocess_per_sketch_from([s.copy() for s in decoded])
    assert out["control_input"].dtype == want.dtype and np.array_equal(out["control_input"], want)
    # a cosine is at most 1: the bound leaves room for the float64 rounding of a quotient of fp32-valued sums
    for key in ("permutation_cosine", "direction_cosine", "time_cosine", "loo_cosine"):
        assert np.isfinite(out[key]).all() and (out[key] <= 1 + 1e-6).all(), key
    # decoded grid sketches lie on multiples of 1/8: the ink of a permuted sketch is the control's ink, exactly
    assert all(np.array_equal(s[:, :2] * 8, np.rint(s[:, :2] * 8)) for s in decoded)
    assert (out["permutation_chamfer"] == 0).all() and (out["direction_chamfer"] == 0).all() and (out["time_chamfer"] == 0).all()
    assert (out["loo_chamfer"] >= 0).all() and np.isfinite(out["permutation_dtw"]).all() and (out["time_dtw"][counts >= 2] > 0).all()
    lists, owner, dropped = strokes.leave_one_out_lists(counts)
    assert np.array_equal(out["loo_owner"], owner) and np.array_equal(out["loo_dropped"], dropped)
    assert np.allclose(out["loo_importance"], out["control_p_true"][owner] - out["loo_p_true"], rtol=0, atol=0)
    assert ((out["loo_share"] > 0) & (out["loo_share"] < 1)).all()
