"""Sequence alignment on the device (skf_align.hip) against the host restatements of tests/align_reference.py: the token edit
distance is an integer and must be equal; every DTW cell is one fixed float32 expression of its neighbours (no fused multiply-add,
a correctly rounded square root, an exact min), so the float32 numpy restatement must be equal too - the raw bits are compared,
nothing here has a tolerance.  Lengths walk the edges of the 64-lane wave and of every strip width the kernel is built for."""
import types

import numpy as np
import pytest
import torch

import align_reference as ref

pytestmark = pytest.mark.gpu

PAD_IDS, PAD_XY = 7, 6                              # columns behind a row's T: ld = T + 7 ids, lda = 2 T + 6 floats


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _id_rows(rng, N, T, vocab=6):
    """(N, T + 7) random ids of a small vocabulary - behind every length, and behind T, lies more of the same (ids that WOULD
    match) - and the (N, T) view the kernel is given"""
    full = _d(rng.randint(1, vocab + 1, size=(N, T + PAD_IDS)).astype(np.int64))
    return full, full[:, :T]


def _point_rows(rng, lengths, T, dyadic=False):
    """(N, 2 T + 6) floats: points uniform in [-1, 1]^2 (or multiples of 1 / 8), NaN behind every length and behind T; the
    (N, T, 2) view the kernel is given; the points as a list of (n, 2) arrays"""
    N = len(lengths)
    pts = rng.randint(-8, 9, size=(N, T, 2)).astype(np.float32) / 8 if dyadic else rng.uniform(-1, 1, size=(N, T, 2)).astype(np.float32)
    full = np.full((N, 2 * T + PAD_XY), np.nan, dtype=np.float32)
    for i, n in enumerate(lengths):
        full[i, :2 * n] = pts[i, :n].reshape(-1)
    dev = _d(full)
    return dev, dev[:, :2 * T].view(N, T, 2), [pts[i, :n] for i, n in enumerate(lengths)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- edit distance
@pytest.mark.parametrize("T", ref.WIDTHS)
def test_edit_distance_paired_over_the_length_grid(T):
    from sketchformer_amd import ops
    pairs = ref.length_pairs(T)
    assert (T < 512 or ((1, 512) in pairs and (512, 1) in pairs)) and (0, 0) in pairs
    S = T // 64                                                   # the strip width of this T: a full and a part-filled last strip
    assert any(lb and lb % S == 0 for _, lb in pairs) and (S == 1 or any(lb % S for _, lb in pairs))
    rng = np.random.RandomState(100 + T)
    N = len(pairs)
    fa, a = _id_rows(rng, N, T)
    fb, b = _id_rows(rng, N, T)
    assert a.stride(0) == T + PAD_IDS and not a.is_contiguous()
    la, lb = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    got = ops.edit_distance(a, b, _d(la), _d(lb))
    assert got.dtype == torch.int32 and tuple(got.shape) == (N,)
    got, ha, hb = got.cpu().numpy(), fa.cpu().numpy(), fb.cpu().numpy()
    want = np.array([ref.edit_distance_ref(ha[i, :la[i]], hb[i, :lb[i]]) for i in range(N)], np.int32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(pairs[i], int(got[i]), int(want[i])) for i in bad[:10]]
    assert np.array_equal(got[(la == 0) | (lb == 0)], np.maximum(la, lb)[(la == 0) | (lb == 0)])       # an empty side: the other's length
    # substitutions, insertions and deletions were all taken: the distances are neither 0 nor the longer length throughout
    both = (la > 2) & (lb > 2)
    assert (got[both] < np.maximum(la, lb)[both]).all() and (got[both] > 0).any()


def test_edit_distance_compares_whole_64_bit_ids():
    from sketchformer_amd import ops
    rng = np.random.RandomState(7)
    T = 70
    base = rng.randint(1, 7, size=(4, T)).astype(np.int64)
    other = base.copy()
    other[0, 5] += 1 << 32                        # differ only above bit 32
    other[1, :] += 1 << 40                        # every id, only above bit 32
    other[2, ::2] |= np.int64(-1) << 33           # sign and high bits
    other[3, 69] += 1 << 62
    n = _d(np.full(4, T, np.int32))
    got = ops.edit_distance(_d(base), _d(other), n, n).cpu().numpy()
    want = [ref.edit_distance_ref(base[i], other[i]) for i in range(4)]
    assert got.tolist() == want and want[0] == 1 and want[1] == T and want[3] == 1


@pytest.mark.parametrize("T", [65, 300])
def test_edit_distance_self_reverse_and_clamped_lengths(T):
    from sketchformer_amd import ops
    rng = np.random.RandomState(T)
    N = 6
    _, a = _id_rows(rng, N, T)
    lens = np.array([T, T - 1, 64, 1, T // 2, T], np.int32)
    assert ops.edit_distance(a, a, _d(lens), _d(lens)).cpu().tolist() == [0] * N            # a row against itself
    ha = a.cpu().numpy()
    rev = np.zeros_like(ha)
    for i in range(N):
        rev[i, :lens[i]] = ha[i, :lens[i]][::-1]
    got = ops.edit_distance(a, _d(rev), _d(lens), _d(lens)).cpu().numpy()
    want = [ref.edit_distance_ref(ha[i, :lens[i]], rev[i, :lens[i]]) for i in range(N)]
    assert got.tolist() == want
    # a length above T is clamped to T, a negative one to 0: never an index
    wild = np.array([T + 1, 1 << 30, -5, T + 7, -(1 << 31), 513], np.int32)
    got = ops.edit_distance(a, _d(rev), _d(wild), _d(lens)).cpu().numpy()
    clamped = np.clip(wild, 0, T)
    want = [ref.edit_distance_ref(ha[i, :clamped[i]], rev[i, :lens[i]]) for i in range(N)]
    assert got.tolist() == want


@pytest.mark.parametrize("Na,Nb", [(3, 5), (5, 3)])
def test_edit_distance_cross_equals_paired(Na, Nb):
    from sketchformer_amd import ops
    rng = np.random.RandomState(10 * Na + Nb)
    Ta, Tb = 200, 130                                             # two widths: a is not b's shape
    fa, a = _id_rows(rng, Na, Ta)
    fb, b = _id_rows(rng, Nb, Tb)
    la, lb = np.array([200, 0, 65, 129, 1][:Na], np.int32), np.array([130, 63, 0, 128, 2][:Nb], np.int32)
    got = ops.edit_distance(a, b, _d(la), _d(lb), cross=True)
    assert tuple(got.shape) == (Na, Nb) and got.dtype == torch.int32
    again = ops.edit_distance(a, b, _d(la), _d(lb), cross=True)
    assert torch.equal(got, again)                                 # two calls agree bit for bit
    got = got.cpu().numpy()
    ha, hb = fa.cpu().numpy(), fb.cpu().numpy()
    want = np.array([[ref.edit_distance_ref(ha[i, :la[i]], hb[j, :lb[j]]) for j in range(Nb)] for i in range(Na)])
    assert np.array_equal(got, want)
    # entry for entry what the paired call gives: row i of a against every row of b
    for i in range(Na):
        rows = a[i:i + 1].expand(Nb, Ta)                           # stride 0 between the rows: one row, Nb times
        paired = ops.edit_distance(rows.contiguous(), b, _d(np.full(Nb, la[i], np.int32)), _d(lb))
        assert np.array_equal(paired.cpu().numpy(), got[i])


# ---------------------------------------------------------------- dynamic time warping
@pytest.mark.parametrize("T", ref.WIDTHS)
def test_dtw_paired_over_the_length_grid_bit_for_bit(T):
    from sketchformer_amd import ops
    pairs = ref.length_pairs(T)
    rng = np.random.RandomState(200 + T)
    N = len(pairs)
    la, lb = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    fa, a, pa = _point_rows(rng, la, T)
    fb, b, pb = _point_rows(rng, lb, T)
    assert a.stride(0) == 2 * T + PAD_XY and tuple(a.shape) == (N, T, 2)
    got = ops.dtw_distance(a, _d(la), b, _d(lb))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N,)
    got = got.cpu().numpy()
    want = np.array([ref.dtw_ref(pa[i], pb[i]) for i in range(N)], np.float32)
    assert np.isfinite(got).all()                                  # the NaNs behind every length were never read into a result
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, [(pairs[i], float(got[i]), float(want[i])) for i in bad[:10]]
    # empty sides, on either or both ends, stand for the point (0, 0)
    empty_a, empty_b = np.nonzero((la == 0) & (lb == 2))[0][0], np.nonzero((la == 2) & (lb == 0))[0][0]
    assert _bits(got[empty_a]) == _bits(ref.dtw_ref_cells(np.zeros((1, 2)), pb[empty_a]))
    assert _bits(got[empty_b]) == _bits(ref.dtw_ref_cells(pa[empty_b], np.zeros((1, 2))))
    assert got[np.nonzero((la == 0) & (lb == 0))[0][0]] == 0.0


def test_dtw_exact_sums_self_and_symmetry():
    from sketchformer_amd import ops
    rng = np.random.RandomState(17)
    T = 130
    lens = np.array([130, 129, 65, 64, 1, 2, 0, 100], np.int32)
    lens_b = np.array([100, 130, 64, 65, 130, 0, 2, 1], np.int32)
    _, a, pa = _point_rows(rng, lens, T, dyadic=True)
    _, b, pb = _point_rows(rng, lens_b, T, dyadic=True)
    got = ops.dtw_distance(a, _d(lens), b, _d(lens_b)).cpu().numpy()
    want = np.array([ref.dtw_ref(p, q) for p, q in zip(pa, pb)], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    back = ops.dtw_distance(b, _d(lens_b), a, _d(lens)).cpu().numpy()                      # symmetric in its arguments, bit for bit
    assert np.array_equal(_bits(back), _bits(got))
    assert not ops.dtw_distance(a, _d(lens), a, _d(lens)).cpu().numpy().any()              # a row with itself: exactly 0.0
    wild = np.array([1 << 30, 129, 65, 64, 1, 2, -4, 100], np.int32)                       # lengths are clamped to [0, T]
    assert np.array_equal(_bits(ops.dtw_distance(a, _d(wild), b, _d(lens_b)).cpu().numpy()), _bits(got))


@pytest.mark.parametrize("Na,Nb", [(3, 5), (5, 3)])
def test_dtw_cross_equals_paired(Na, Nb):
    from sketchformer_amd import ops
    rng = np.random.RandomState(20 * Na + Nb)
    Ta, Tb = 64, 260
    la, lb = np.array([64, 0, 63, 1, 2][:Na], np.int32), np.array([260, 129, 0, 200, 65][:Nb], np.int32)
    _, a, pa = _point_rows(rng, la, Ta)
    _, b, pb = _point_rows(rng, lb, Tb)
    got = ops.dtw_distance(a, _d(la), b, _d(lb), cross=True)
    assert tuple(got.shape) == (Na, Nb) and got.dtype == torch.float32
    assert torch.equal(got, ops.dtw_distance(a, _d(la), b, _d(lb), cross=True))
    got = got.cpu().numpy()
    want = np.array([[ref.dtw_ref(p, q) for q in pb] for p in pa], np.float32)
    assert np.array_equal(_bits(got), _bits(want))
    swapped = ops.dtw_distance(b, _d(lb), a, _d(la), cross=True).cpu().numpy()             # the strips on the other operand
    assert np.array_equal(_bits(swapped), _bits(want.T))
    for i in range(Na):
        rows = a[i:i + 1].expand(Nb, Ta, 2).contiguous()
        paired = ops.dtw_distance(rows, _d(np.full(Nb, la[i], np.int32)), b, _d(lb)).cpu().numpy()
        assert np.array_equal(_bits(paired), _bits(got[i]))


def test_library_refusals():
    import ctypes as C
    from sketchformer_amd import _lib
    lib = _lib.load()
    ids, n, out = torch.ones(4, 600, dtype=torch.int64).cuda(), torch.ones(4, dtype=torch.int32).cuda(), torch.zeros(16, dtype=torch.int32).cuda()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                                      # noqa: E731

    def edit(lda=600, Na=4, Ta=8, ldb=600, Nb=4, Tb=8, cross=0, a_off=0):
        return lib.skf_edit_distance_i64(P(ids, a_off), lda, P(n), Na, Ta, P(ids), ldb, P(n), Nb, Tb, cross, P(out), None)
    assert edit() == 0
    for bad in (dict(Na=0), dict(Ta=0), dict(Ta=513), dict(Tb=513), dict(lda=7), dict(ldb=7), dict(Nb=3), dict(a_off=4), dict(cross=2)):
        assert edit(**bad) != 0, bad
    assert edit(Nb=3, cross=1) == 0
    xy, fout = torch.zeros(4, 1200).cuda(), torch.zeros(16).cuda()

    def dtw(lda=1200, Na=4, Ta=8, ldb=1200, Nb=4, Tb=8, cross=0, a_off=0):
        return lib.skf_dtw_f32(P(xy, a_off), lda, P(n), Na, Ta, P(xy), ldb, P(n), Nb, Tb, cross, P(fout), None)
    assert dtw() == 0
    for bad in (dict(Nb=0), dict(Tb=0), dict(Ta=513), dict(lda=15), dict(ldb=15), dict(Na=3), dict(a_off=2)):
        assert dtw(**bad) != 0, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- front ends
def _dyadic_dict_tokenizer(tmp_path, K, L):
    from sketchformer_amd.utils.tokenizer import Tokenizer
    path = str(tmp_path / "dict.npz")
    centers = np.random.RandomState(3).randint(-48, 49, size=(K, 2)).astype(np.float32) / 1024.0      # partial sums stay exact
    np.savez(path, cluster_centers=centers, inertia=np.float64(0), n_iter=np.int64(1))
    return Tokenizer(path, max_seq_len=L)


def _synthetic_stroke3(n, seed):
    """n sketches of sketchformer_amd/synthetic.py as stroke-3 rows, scaled into the unit box as the loader scales them"""
    from sketchformer_amd import synthetic
    from sketchformer_amd.metrics.samples import stroke5_to_stroke3
    x, _ = synthetic.continuous_batch(n, seq_len=120, seed=seed)
    out = []
    for row in x:
        s3 = np.asarray(stroke5_to_stroke3(row), dtype=np.float32)
        pos = np.cumsum(s3[:, :2].astype(np.float64), axis=0)
        s3[:, :2] /= np.float32(max(np.ptp(np.r_[pos[:, 0], 0]), np.ptp(np.r_[pos[:, 1], 0]), 1e-3))
        out.append(s3)
    return out


def test_front_ends_through_the_real_tokenizers(tmp_path):
    from sketchformer_amd import align
    from sketchformer_amd.utils.tokenizer import GridTokenizer
    L = 100
    sketches = _synthetic_stroke3(8, seed=5)
    assert len({len(s) for s in sketches}) > 3
    for tok in (GridTokenizer(resolution=16, max_seq_len=L), _dyadic_dict_tokenizer(tmp_path, 40, L)):
        a = np.stack([tok.encode(s) for s in sketches])                              # some rows truncated, some padded
        b = np.stack([tok.encode(s[::2]) for s in sketches[1:] + sketches[:1]])      # other sketches, thinned out
        b[3] = a[3]
        assert a.shape == (8, L) and 0 < (a[:, -1] == tok.PAD).sum() < 8        # padded rows and rows cut at max_seq_len
        sa, sb = [ref.token_span_ref(r, tok) for r in a], [ref.token_span_ref(r, tok) for r in b]
        want = np.array([ref.edit_distance_ref(p, q) for p, q in zip(sa, sb)])
        got = align.token_edit_distance(a, b, tok)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and want[3] == 0 and want.max() > 10
        rate = align.token_edit_distance(a, b, tok, normalize=True)
        longer = np.array([max(len(p), len(q), 1) for p, q in zip(sa, sb)], np.float64)
        assert rate.dtype == torch.float64 and np.array_equal(rate.cpu().numpy(), want / longer) and float(rate.max()) <= 1.0
        cross = align.token_edit_distance(a[:3], b, tok, cross=True).cpu().numpy()
        assert cross.shape == (3, 8) and np.array_equal(cross, [[ref.edit_distance_ref(p, q) for q in sb] for p in sa[:3]])
        pa, pb = [ref.decoded_points(r, tok) for r in a], [ref.decoded_points(r, tok) for r in b]
        want = np.array([ref.dtw_ref(p, q) for p, q in zip(pa, pb)], np.float32)
        got = align.sketch_dtw(a, b, kind="tokens", tokenizer=tok, normalize=False)
        assert got.dtype == torch.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and want[3] == 0 and want.max() > 1
        steps = np.array([len(p) + len(q) for p, q in zip(pa, pb)], np.float64)
        norm = align.sketch_dtw(a, b, kind="tokens", tokenizer=tok)
        assert norm.dtype == torch.float64 and np.array_equal(norm.cpu().numpy(), want.astype(np.float64) / steps)
        cross = align.sketch_dtw(a[:3], b, kind="tokens", tokenizer=tok, cross=True, normalize=False).cpu().numpy()
        assert np.array_equal(_bits(cross), _bits(np.array([[ref.dtw_ref(p, q) for q in pb] for p in pa[:3]], np.float32)))


def test_metrics_on_hand_built_predictions():
    from sketchformer_amd import metrics
    from sketchformer_amd.metrics.samples import stroke5_to_stroke3
    from sketchformer_amd.utils.tokenizer import GridTokenizer
    import raster_reference as rr
    # token model: 4 originals (B, L), 4 reconstructions (B, L + 1) as the greedy decoder returns them
    tok, L = GridTokenizer(resolution=16, max_seq_len=40), 40
    sketches = _synthetic_stroke3(8, seed=9)
    x = np.stack([tok.encode(s[:30]) for s in sketches[:4]])
    pred = np.zeros((4, L + 1), np.int64)
    pred[:, :L] = np.stack([tok.encode(s[:25:2]) for s in sketches[4:]])
    pred[1, :L] = x[1]                                                                  # one perfect reconstruction
    pred[2] = 0
    pred[2, 0] = tok.SOS                                                                # one that emitted nothing
    data = (x, None, pred, None, None, tok, None, None, False)
    sa, sb = [ref.token_span_ref(r, tok) for r in x], [ref.token_span_ref(r, tok) for r in pred]
    want = np.mean([ref.edit_distance_ref(p, q) / max(len(p), len(q), 1) for p, q in zip(sa, sb)])
    value = metrics.build_metric_by_name("recon-token-error", {}).compute(data)
    assert isinstance(value, float) and abs(value - want) <= 1e-12 and 0.25 < value < 1.0
    pa, pb = [ref.decoded_points(r, tok) for r in x], [ref.decoded_points(r, tok) for r in pred]
    assert len(pb[2]) == 1 and not pb[2].any()                                          # the host's dummy row of an empty sketch
    want = np.mean([np.float64(ref.dtw_ref(p, q)) / (len(p) + len(q)) for p, q in zip(pa, pb)])
    value = metrics.build_metric_by_name("recon-dtw", {}).compute(data)
    assert isinstance(value, float) and abs(value - want) <= 1e-12 and value > 0
    # continuous model: stroke-5 rows with dyadic offsets (their sums are exact); pred_x carries the start row, the originals do not
    T = 65
    cases = rr.stroke5_cases(T, 31 + T)
    s5 = np.stack([cases[k] for k in ("no_end", "end_middle", "end_first", "tie_lift_end")])
    other = s5[[1, 0, 3, 2]]
    pred = np.concatenate([np.zeros((4, 1, 5), np.float32), other], axis=1)
    pred[:, 0, 2] = 1.0
    data = (s5, None, pred, None, None, None, None, None, True)

    def pts(rows):
        return np.cumsum(np.asarray(stroke5_to_stroke3(rows), np.float64).reshape(-1, 3)[:, :2], axis=0).astype(np.float32)
    want = np.mean([np.float64(ref.dtw_ref(pts(p), pts(q))) / (max(len(pts(p)), 1) + max(len(pts(q)), 1)) for p, q in zip(s5, other)])
    value = metrics.build_metric_by_name("recon-dtw", {}).compute(data)
    assert abs(value - want) <= 1e-12 and value > 0
    assert metrics.build_metric_by_name("recon-dtw", {}).compute((s5, None, np.concatenate([pred[:, :1], s5], axis=1)) + data[3:]) == 0.0
    with pytest.raises(ValueError, match="continuous"):
        metrics.build_metric_by_name("recon-token-error", {}).compute(data)


@pytest.mark.parametrize("distance,sets", [("edit", "gallery_set=test,query_set=valid"), ("dtw", "gallery_set=test,query_set=valid"),
                                           ("edit", "gallery_set=valid,query_set=valid")])
def test_sequence_retrieval_experiment(tmp_path, distance, sets):
    from sketchformer_amd import dataloaders, experiments, retrieval
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=4,n_samples=64"), None)
    model = types.SimpleNamespace(dataset=dataset)                  # the experiment uses model.dataset only
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    exp = Exp(Exp.parse_hparams("distance=%s,n_queries=8,n_gallery=32,top_k=5,gallery_block=12,%s" % (distance, sets)), "s0", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    assert {"indices", "distances", "query_y", "gallery_y", "query_rows", "map_at_k", "precision_at_k", "recall_at_1", "per_class_ap",
            "class_names"} <= set(out.files)                         # the keys of retrieval.npz
    assert out["indices"].shape == (8, 5) and out["indices"].dtype == np.int32 and out["distances"].shape == (8, 5)
    assert out["gallery_y"].shape == (32,) and out["query_y"].shape == (8,) and out["per_class_ap"].shape == (4,)
    same = "gallery_set=valid" in sets
    tok = dataset.tokenizer
    gx, gy = dataset.get_all_data_from("valid" if same else "test")
    gx, gy = gx[out["gallery_rows"]], gy.reshape(-1)[out["gallery_rows"]]
    assert np.array_equal(gy, out["gallery_y"]) and len(np.unique(out["gallery_rows"])) == 32
    if same:
        pos = np.searchsorted(out["gallery_rows"], out["query_rows"])
        assert np.array_equal(out["gallery_rows"][pos], out["query_rows"])           # the queries come from the ranked gallery
        qx = gx[pos]
    else:
        qx = dataset.get_all_data_from("valid")[0][out["query_rows"]]
    if distance == "edit":
        D = np.array([[ref.edit_distance_ref(ref.token_span_ref(q, tok), ref.token_span_ref(g, tok)) for g in gx] for q in qx], np.float32)
    else:
        D = np.array([[ref.dtw_ref(ref.decoded_points(q, tok), ref.decoded_points(g, tok)) for g in gx] for q in qx], np.float32)
    if same:
        assert (D[np.arange(8), pos] == 0).all()
        D[np.arange(8), pos] = np.inf                                # leave-one-out
    want = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert np.array_equal(out["indices"], want)
    assert np.array_equal(_bits(out["distances"]), _bits(np.take_along_axis(D, want, axis=1)))
    scores = retrieval.retrieval_scores(want, out["query_y"], gy, exclude_self=same)
    assert float(out["map_at_k"]) == scores["map_at_k"] and float(out["recall_at_1"]) == scores["recall_at_1"]
