"""Host side of the sequence-alignment feature: the restatements of tests/align_reference.py on cases whose answers are known by
hand, the token-span rule of sketchformer_amd/align.py against its restatement on rows of the real tokenizers, the ranking
helper, the plugin registries and the refusals of the wrappers.  Nothing here needs a device."""
import numpy as np
import pytest

import align_reference as ref


def _align():
    from sketchformer_amd import align
    return align


def _ids(word):
    return [ord(c) for c in word]


# ---------------------------------------------------------------- the restatements on known answers
def test_edit_distance_reference_on_known_answers():
    _align()                                             # (the feature these references restate must exist)
    assert ref.edit_distance_ref(_ids("kitten"), _ids("sitting")) == 3
    assert ref.edit_distance_ref(_ids("flaw"), _ids("lawn")) == 2
    assert ref.edit_distance_ref(_ids("sunday"), _ids("saturday")) == 3
    row = list(range(1, 40))
    assert ref.edit_distance_ref(row, row) == 0
    assert ref.edit_distance_ref(range(10), range(100, 117)) == 17 and ref.edit_distance_ref(range(100, 117), range(10)) == 17
    for n in (0, 1, 7):
        assert ref.edit_distance_ref([], range(n)) == n and ref.edit_distance_ref(range(n), []) == n
    assert ref.edit_distance_ref([1, 2, 3, 4], [2, 3, 4]) == 1 and ref.edit_distance_ref([1, 2, 3, 4], [1, 2, 4]) == 1
    assert ref.edit_distance_ref([1 << 40], [(1 << 40) + (1 << 33)]) == 1          # ids are whole integers, not their low words
    rng = np.random.RandomState(3)
    for _ in range(20):                                                          # symmetric, and bounded by the longer side
        a, b = rng.randint(1, 5, size=rng.randint(0, 30)), rng.randint(1, 5, size=rng.randint(0, 30))
        d = ref.edit_distance_ref(a, b)
        assert d == ref.edit_distance_ref(b, a) and abs(len(a) - len(b)) <= d <= max(len(a), len(b))


def test_dtw_reference_on_known_answers():
    _align()
    rng = np.random.RandomState(5)
    a = rng.uniform(-1, 1, size=(37, 2)).astype(np.float32)
    assert ref.dtw_ref(a, a) == 0.0 and ref.dtw_ref(a, a).dtype == np.float32
    # by hand: a = (0,0) (3,4) (6,8), b = (0,0) (6,8).  c = [[0, 10], [5, 5], [10, 0]];
    # D = [[0, 10], [5, 5], [15, 5]]: (0,0) -> (1,0) or (1,1) -> (2,1), total 5
    a3, b2 = [[0, 0], [3, 4], [6, 8]], [[0, 0], [6, 8]]
    assert np.array_equal(ref.local_cost(a3, b2), [[0, 10], [5, 5], [10, 0]])
    assert ref.dtw_ref(a3, b2) == 5.0 and ref.dtw_ref_cells(a3, b2) == 5.0
    # a single point against a row: the sum of the distances (a border is a running sum)
    assert ref.dtw_ref([[0, 0]], [[3, 4], [0, 1], [6, 8]]) == 16.0
    # an empty side is the point (0, 0); both empty: 0
    assert ref.dtw_ref(np.zeros((0, 2)), [[3, 4], [6, 8]]) == 15.0 and ref.dtw_ref([[3, 4], [6, 8]], []) == 15.0
    assert ref.dtw_ref([], []) == 0.0
    # symmetric in its arguments, bit for bit (c is, and min does not care for the order), and the two sweeps agree bit for bit
    for na, nb in ((1, 1), (2, 9), (9, 2), (17, 23), (64, 65)):
        p = rng.uniform(-1, 1, size=(na, 2)).astype(np.float32)
        q = rng.uniform(-1, 1, size=(nb, 2)).astype(np.float32)
        d = ref.dtw_ref(p, q)
        assert d.tobytes() == ref.dtw_ref(q, p).tobytes() == ref.dtw_ref_cells(p, q).tobytes()
        assert d > 0 and d.dtype == np.float32


# ---------------------------------------------------------------- token spans
def _dict_tokenizer(tmp_path, K=12, max_seq_len=0):
    from sketchformer_amd.utils.tokenizer import Tokenizer
    path = str(tmp_path / "dict.npz")
    centers = np.random.RandomState(7).randint(-48, 49, size=(K, 2)).astype(np.float32) / 1024.0
    np.savez(path, cluster_centers=centers, inertia=np.float64(0), n_iter=np.int64(1))
    return Tokenizer(path, max_seq_len=max_seq_len)


def _sketch(rng, n):
    s = np.c_[rng.uniform(-0.02, 0.02, size=(n, 2)), (rng.rand(n) < 0.2)].astype(np.float32)
    s[-1, 2] = 1
    return s


def _check_spans(align, rows, tok):
    import torch
    view, lengths = align.token_spans(rows, tok)
    assert torch.is_tensor(view) and view.dtype == torch.int64 and lengths.dtype == torch.int32 and lengths.shape == (len(rows),)
    for i, row in enumerate(rows):
        want = ref.token_span_ref(row, tok)
        assert int(lengths[i]) == len(want), (i, int(lengths[i]), len(want))
        assert view[i, :len(want)].tolist() == want, i
    return view, lengths


def test_token_spans_follow_the_reference_rule(tmp_path):
    import torch
    align = _align()
    from sketchformer_amd.utils.tokenizer import GridTokenizer
    rng = np.random.RandomState(11)
    L = 24
    for tok in (_dict_tokenizer(tmp_path, max_seq_len=L), GridTokenizer(resolution=16, max_seq_len=L)):
        rows = np.stack([tok.encode(_sketch(rng, n)) for n in (3, 9, 15, 40)])          # the last one is truncated by the tokenizer
        assert rows.shape == (4, L) and (rows[:, 0] == tok.SOS).all()
        view, lengths = _check_spans(align, rows, tok)
        # every row leads with SOS: a view from column 1 into the rows, not a copy
        assert tuple(view.shape) == (4, L - 1) and view.stride(0) == L and view.data_ptr() == torch.from_numpy(rows)[:, 1:].data_ptr()
        full = rows[3].copy()
        full[1:] = np.where(np.isin(full[1:], (tok.EOS, tok.PAD)), 1, full[1:])      # a truncated row without EOS: to the row's end
        special = np.stack([full,
                            np.full(L, tok.PAD),                                      # all PAD
                            np.r_[tok.SOS, tok.EOS, np.full(L - 2, tok.PAD)],         # SOS and EOS only
                            np.r_[tok.SOS, tok.SOS, 1, 2, tok.EOS, np.full(L - 5, tok.PAD)],   # only ONE leading SOS is dropped
                            np.r_[1, 2, 3, tok.EOS, 4, 5, np.full(L - 6, tok.PAD)]])  # no SOS; what follows EOS is not content
        view, lengths = _check_spans(align, special, tok)                             # a mixed batch: a shifted copy
        assert lengths.tolist() == [L - 1, 0, 0, 3, 3]
        assert ref.token_span_ref(special[3], tok) == [tok.SOS, 1, 2]
        view, lengths = _check_spans(align, special[[1, 4]], tok)                     # no row leads with SOS: the rows themselves
        assert tuple(view.shape) == (2, L)
        view, _ = _check_spans(align, rows[:, :, None], tok)                          # (N, L, 1) token columns of the file loaders
        assert tuple(view.shape) == (4, L - 1)
    with pytest.raises(ValueError):
        align.token_spans(np.zeros((2, 3, 4), np.int64), tok)


# ---------------------------------------------------------------- ranking
def test_rank_by_distance_ties_exclusion_and_clamp():
    import torch
    align = _align()
    D = np.array([[3, 1, 1, 0, 1],
                  [2, 2, 2, 2, 2],
                  [0, 5, 4, 4, 9]], dtype=np.float32)
    idx, dist = align.rank_by_distance(D, 3)
    assert idx.dtype == np.int32 and idx.tolist() == [[3, 1, 2], [0, 1, 2], [0, 2, 3]]       # equal distances: gallery-row order
    assert dist.dtype == np.float32 and dist.tolist() == [[0, 1, 1], [2, 2, 2], [0, 4, 4]]
    idx, dist = align.rank_by_distance(torch.from_numpy(D), 3, exclude_rows=[3, 0, -1])      # one row left out per query; -1: none
    assert idx.tolist() == [[1, 2, 4], [1, 2, 3], [0, 2, 3]] and dist.tolist() == [[1, 1, 1], [2, 2, 2], [0, 4, 4]]
    idx, _ = align.rank_by_distance(D, 99)
    assert idx.shape == (3, 5) and idx[1].tolist() == [0, 1, 2, 3, 4]                        # k clamped to the gallery
    idx, _ = align.rank_by_distance(D, 99, exclude_rows=np.array([0, 1, 2]))
    assert idx.shape == (3, 4) and idx.tolist() == [[3, 1, 2, 4], [0, 2, 3, 4], [0, 3, 1, 4]]     # ... minus the excluded row
    idx, dist = align.rank_by_distance(D.astype(np.int32), 2)                                # integer distances keep their type
    assert dist.dtype == np.int32 and idx.tolist() == [[3, 1], [0, 1], [0, 2]]
    from sketchformer_amd import retrieval
    scores = retrieval.retrieval_scores(idx, np.array([0, 1, 0]), np.array([0, 1, 0, 0, 1]))  # the layout retrieval_scores takes
    assert scores["n_queries_scored"] == 3 and scores["recall_at_1"] == pytest.approx(2.0 / 3.0)
    with pytest.raises(ValueError):
        align.rank_by_distance(np.zeros(5), 2)
    with pytest.raises(ValueError):
        align.rank_by_distance(D, 2, exclude_rows=[0, 1])
    with pytest.raises(ValueError):
        align.rank_by_distance(D[:, :1], 1, exclude_rows=[0, 0, 0])


# ---------------------------------------------------------------- the plugin surface
def test_plugins_are_registered_and_their_hparams_parse():
    _align()
    from sketchformer_amd import experiments, metrics
    for name in ("recon-token-error", "recon-dtw"):
        metric = metrics.build_metric_by_name(name, {})
        assert metric.name == name and metric.input_type == "predictions_on_validation_set"
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    assert Exp.requires_model
    h = dict(Exp.default_hparams().values())
    assert (h["distance"], h["gallery_set"], h["query_set"], h["top_k"]) == ("dtw", "test", "valid", 100)
    assert (h["n_queries"], h["n_gallery"], h["target_file"]) == (256, 4096, "sequence_retrieval.npz") and h["gallery_block"] >= 1
    h = dict(Exp.parse_hparams("distance=edit,n_queries=8,n_gallery=32,top_k=5,gallery_block=16").values())
    assert (h["distance"], h["n_queries"], h["n_gallery"], h["top_k"], h["gallery_block"]) == ("edit", 8, 32, 5, 16)
    # a continuous model has no token ids to compare
    s5 = np.zeros((2, 4, 5), np.float32)
    with pytest.raises(ValueError, match="continuous"):
        metrics.build_metric_by_name("recon-token-error", {}).compute((s5, None, s5, None, None, None, None, None, True))
    with pytest.raises(ValueError, match="reconstructions"):
        metrics.build_metric_by_name("recon-dtw", {}).compute((s5[:0], None, s5[:0], None, None, None, None, None, True))


# ---------------------------------------------------------------- refusals of the wrappers
def test_wrappers_refuse_host_tensors_and_malformed_operands():
    import torch
    _align()
    from sketchformer_amd import _lib, ops
    assert ops.ALIGN_MAX_LEN == 512
    a, la = torch.ones(3, 8, dtype=torch.int64), torch.full((3,), 8, dtype=torch.int32)
    xy, n = torch.zeros(3, 8, 2), torch.full((3,), 8, dtype=torch.int32)
    # no CPU path: well-formed host tensors are refused with SkfError
    with pytest.raises(_lib.SkfError):
        ops.edit_distance(a, a, la, la)
    with pytest.raises(_lib.SkfError):
        ops.edit_distance(a, a[:2], la, la[:2], cross=True)
    with pytest.raises(_lib.SkfError):
        ops.dtw_distance(xy, n, xy, n)
    with pytest.raises(_lib.SkfError):
        ops.dtw_distance(xy, n, xy[:1], n[:1], cross=True)
    # a wrong dtype
    with pytest.raises(TypeError):
        ops.edit_distance(a.to(torch.int32), a, la, la)
    with pytest.raises(TypeError):
        ops.edit_distance(a, a, la.to(torch.int64), la)
    with pytest.raises(TypeError):
        ops.dtw_distance(xy.double(), n, xy, n)
    with pytest.raises(TypeError):
        ops.dtw_distance(xy, n, xy, n.to(torch.int64))
    with pytest.raises(TypeError):
        ops.dtw_distance(torch.zeros(3, 8, 3), n, xy, n)                          # (x, y, pen) rows are not points
    # a non-unit stride
    with pytest.raises(ValueError):
        ops.edit_distance(torch.ones(3, 16, dtype=torch.int64)[:, ::2], a, la, la)
    with pytest.raises(ValueError):
        ops.dtw_distance(torch.zeros(3, 8, 4)[:, :, ::2], n, xy, n)
    with pytest.raises(ValueError):
        ops.dtw_distance(torch.zeros(3, 16, 2)[:, ::2], n, xy, n)
    # mismatched N without cross
    with pytest.raises(ValueError, match="paired"):
        ops.edit_distance(a, a[:2], la, la[:2])
    with pytest.raises(ValueError, match="paired"):
        ops.dtw_distance(xy, n, xy[:2], n[:2])
    # rows longer than the limit
    big, lb = torch.ones(3, 513, dtype=torch.int64), torch.full((3,), 513, dtype=torch.int32)
    with pytest.raises(ValueError, match="512"):
        ops.edit_distance(big, a, lb, la)
    with pytest.raises(ValueError, match="512"):
        ops.dtw_distance(xy, n, torch.zeros(3, 513, 2), n)
