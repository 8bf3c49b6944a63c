"""Order-free shape distances on the device (skf_chamfer.hip) against the float32 restatement of tests/shape_reference.py.  Every
operation of the rule is rounded on its own, the minimum and the maximum are exact and the mean is a fixed-point sum, so the four
outputs of a pair must be equal to the restatement's - the raw bits are compared, nothing here has a tolerance.  Lengths walk the
empty sketch, the shortest rows and the edges of a 64-lane wave and of the 256-thread workgroup (n * S around 256 and 512)."""
import types

import numpy as np
import pytest
import torch

import shape_reference as ref

pytestmark = pytest.mark.gpu

PAD_XY, PAD_PEN = 6, 5                              # columns behind a row's T: lda = 2 T + 6 floats, ldp = T + 5 bytes
T_SMALL = 130


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _sketches(rng, lengths, pattern):
    """one (points (n, 2) float32, pen (n,) uint8) per length, of a pen / point pattern"""
    out = []
    for n in lengths:
        xy = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        pen = (rng.uniform(size=n) < 0.2).astype(np.uint8)
        if pattern == "lifted":                                    # dots only
            pen[:] = 1
        elif pattern == "joined":                                  # one stroke
            pen[:] = 0
            pen[-1:] = 1
        elif pattern == "repeated":                                # every point twice or three times: segments with len2 = 0
            xy = np.repeat(xy[:(n + 2) // 3], 3, axis=0)[:n]
            pen[:] = rng.uniform(size=n) < 0.1
        elif pattern == "collinear":                               # runs of points on one line, forwards and backwards
            step = rng.randint(-3, 4, size=(n, 1)).astype(np.float32)
            line = rng.randint(-8, 9, size=(2, 2)).astype(np.float32) / 64          # a direction and an origin of its own
            xy = (np.cumsum(step, axis=0) * line[:1] + line[1:]).astype(np.float32)
            pen[:] = rng.uniform(size=n) < 0.05
        elif pattern == "grid255":                                 # the integer grid of the simplified QuickDraw files
            xy = rng.randint(0, 256, size=(n, 2)).astype(np.float32)
        else:
            assert pattern == "random"
        out.append((xy, pen))
    return out


def _pack(sketches, T, fill=np.nan, pen_fill=0):
    """device rows with pitches larger than their width: xy (N, T, 2) inside (N, 2 T + 6) floats, pen (N, T) inside (N, T + 5) bytes,
    `fill` / `pen_fill` behind every length and behind T (NaN: nothing there may reach a result); n (N,) int32"""
    N = len(sketches)
    xy = np.full((N, 2 * T + PAD_XY), fill, dtype=np.float32)
    pen = np.full((N, T + PAD_PEN), pen_fill, dtype=np.uint8)
    for i, (p, q) in enumerate(sketches):
        xy[i, :2 * len(p)] = p.reshape(-1)
        pen[i, :len(q)] = q
    dx, dp = _d(xy), _d(pen)
    vx, vp = dx[:, :2 * T].view(N, T, 2), dp[:, :T]
    assert N == 1 or (vx.stride(0) == 2 * T + PAD_XY and vp.stride(0) == T + PAD_PEN)
    return vx, vp, _d(np.array([len(p) for p, _ in sketches], np.int32))


def _want(A, B, S, cross=False):
    if cross:
        return np.array([[ref.shape_ref(a[0], a[1], b[0], b[1], S) for b in B] for a in A], np.float32)
    return np.array([ref.shape_ref(a[0], a[1], b[0], b[1], S) for a, b in zip(A, B)], np.float32)


def _assert_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:8]])


# ---------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("pattern", ["lifted", "joined", "random", "repeated", "collinear", "grid255"])
def test_paired_bit_for_bit(pattern, S):
    from sketchformer_amd import ops
    rng = np.random.RandomState(len(pattern) * 100 + S)
    la = list(ref.LENGTHS) * 2
    lb = list(ref.LENGTHS[3:] + ref.LENGTHS[:3]) + list(ref.LENGTHS[::-1])         # every length meets others, 0 meets 0 never ...
    la, lb = la + [0, 130], lb + [0, 130]                                           # ... so: both empty, both full
    A, B = _sketches(rng, la, pattern), _sketches(rng, lb, pattern)
    xa, pa, na = _pack(A, T_SMALL)
    xb, pb, nb = _pack(B, T_SMALL)
    got = ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(la), 4)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()                                  # the NaNs behind every length were never read into a result
    want = _want(A, B, S)
    _assert_bits(got, want, (pattern, S))
    assert not got[-2].any()                                       # empty against empty: the point (0, 0) against itself
    if pattern in ("lifted", "joined", "random", "repeated"):      # points drawn from the plane: no ink of one lies on the other's
        assert (got[[i for i in range(len(la)) if la[i] > 3 and lb[i] > 3]] > 0).all()
    if pattern == "lifted":                                        # no segment: S plays no part
        _assert_bits(got, _want(A, B, 1), "dots only")


def test_one_pair_at_the_longest_row():
    from sketchformer_amd import ops
    rng = np.random.RandomState(512)
    A, B = _sketches(rng, [512], "random"), _sketches(rng, [512], "grid255")
    B = [(B[0][0] / np.float32(128) - np.float32(1), B[0][1])]
    xa, pa, na = _pack(A, 512)
    xb, pb, nb = _pack(B, 512)
    for S in (1, 4, 16):
        _assert_bits(ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=S), _want(A, B, S), S)


def test_lengths_are_clamped_and_never_an_index():
    from sketchformer_amd import ops
    rng = np.random.RandomState(9)
    T = 65
    A, B = _sketches(rng, [T] * 6, "random"), _sketches(rng, [T, 64, 1, 0, 33, T], "random")
    xa, pa, _ = _pack(A, T)
    xb, pb, nb = _pack(B, T)
    wild = np.array([T + 1, 1 << 30, -5, T + 7, -(1 << 31), 513], np.int32)
    clamped = np.clip(wild, 0, T)
    got = ops.shape_distance(xa, pa, _d(wild), xb, pb, nb, samples_per_segment=4)
    _assert_bits(got, _want([(p[:n], q[:n]) for (p, q), n in zip(A, clamped)], B, 4), "wild n_a")
    back = ops.shape_distance(xb, pb, nb, xa, pa, _d(wild), samples_per_segment=4).cpu().numpy()
    _assert_bits(back[:, [1, 0, 3, 2]], got.cpu().numpy(), "wild n_b, sides swapped")


@pytest.mark.parametrize("Na,Nb", [(3, 5), (2, 9)])
def test_cross_bit_for_bit_and_equal_to_paired(Na, Nb):
    from sketchformer_amd import ops
    assert ops.SHAPE_GALLERY_BLOCK == 8                            # (2, 9): one row more than a workgroup's block of gallery rows
    rng = np.random.RandomState(10 * Na + Nb)
    Ta, Tb = 65, T_SMALL
    la, lb = [65, 0, 64][:Na], [130, 63, 0, 128, 2, 1, 127, 3, 129][:Nb]
    A, B = _sketches(rng, la, "random"), _sketches(rng, lb, "random")
    xa, pa, na = _pack(A, Ta)
    xb, pb, nb = _pack(B, Tb)
    got = ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=4, cross=True)
    assert tuple(got.shape) == (Na, Nb, 4) and got.dtype == torch.float32
    assert torch.equal(got, ops.shape_distance(xa, pa, na, xb, pb, nb, samples_per_segment=4, cross=True))      # two calls: the same bits
    got = got.cpu().numpy()
    _assert_bits(got, _want(A, B, 4, cross=True), "cross")
    swapped = ops.shape_distance(xb, pb, nb, xa, pa, na, samples_per_segment=4, cross=True).cpu().numpy()
    _assert_bits(swapped.transpose(1, 0, 2)[:, :, [1, 0, 3, 2]], got, "sides swapped")
    # entry for entry what the paired call gives: row i of a against every row of b
    for i in range(Na):
        rows = lambda t: t[i:i + 1].expand(Nb, *t.shape[1:]).contiguous()                  # noqa: E731
        paired = ops.shape_distance(rows(xa), rows(pa), rows(na), xb, pb, nb, samples_per_segment=4)
        _assert_bits(paired, got[i], "paired row %d" % i)


def test_a_row_does_not_depend_on_its_batch_and_garbage_behind_the_length_is_not_read():
    from sketchformer_amd import ops
    rng = np.random.RandomState(21)
    la, lb = [130, 5, 64, 0, 100], [7, 129, 65, 12, 0]
    A, B = _sketches(rng, la, "random"), _sketches(rng, lb, "random")
    clean = [_pack(X, T_SMALL, fill=0.0, pen_fill=0) for X in (A, B)]
    dirty = [_pack(X, T_SMALL, fill=np.nan, pen_fill=255) for X in (A, B)]
    base = ops.shape_distance(*clean[0], *clean[1], samples_per_segment=4)
    assert torch.equal(base, ops.shape_distance(*dirty[0], *dirty[1], samples_per_segment=4))
    assert torch.equal(base, ops.shape_distance(*clean[0], *clean[1], samples_per_segment=4))                  # two calls: the same bits
    for i in range(len(la)):                                       # every pair alone, and in a batch of other neighbours
        one = ops.shape_distance(*(t[i:i + 1] for t in dirty[0]), *(t[i:i + 1] for t in dirty[1]), samples_per_segment=4)
        assert torch.equal(one[0], base[i])
    order = [3, 0, 4, 2, 1]
    moved = ops.shape_distance(*(t[order] for t in clean[0]), *(t[order] for t in clean[1]), samples_per_segment=4)
    assert torch.equal(moved, base[order])
    crossed = ops.shape_distance(*dirty[0], *dirty[1], samples_per_segment=4, cross=True)
    assert torch.equal(torch.stack([crossed[i, i] for i in range(len(la))]), base)


def test_library_refusals():
    import ctypes as C
    from sketchformer_amd import _lib
    lib = _lib.load()
    xy, pen = torch.zeros(4, 1200).cuda(), torch.zeros(4, 600, dtype=torch.uint8).cuda()
    n, out = torch.ones(4, dtype=torch.int32).cuda(), torch.zeros(4 * 4 * 4 + 4).cuda()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                                      # noqa: E731

    def call(lda=1200, ldpa=600, Na=4, Ta=8, ldb=1200, ldpb=600, Nb=4, Tb=8, S=4, cross=0, a_off=0, n_off=0, out_off=0):
        return lib.skf_shape_distance_f32(P(xy, a_off), lda, P(pen), ldpa, P(n, n_off), Na, Ta, P(xy), ldb, P(pen), ldpb, P(n), Nb, Tb, S, cross,
                                          P(out, out_off), None)
    assert call() == 0 and call(Nb=3, cross=1) == 0 and call(S=1) == 0 and call(S=16) == 0 and call(Ta=512, Tb=512) == 0
    for bad in (dict(Na=0), dict(Nb=0), dict(Ta=0), dict(Tb=0), dict(Ta=513), dict(Tb=513), dict(lda=15), dict(ldb=15), dict(ldpa=7),
                dict(ldpb=7), dict(Nb=3), dict(S=0), dict(S=17), dict(cross=2), dict(cross=-1), dict(a_off=2), dict(n_off=2), dict(out_off=4),
                dict(Na=1 << 15, Nb=1 << 14, cross=1)):
        assert call(**bad) != 0, bad
        assert b"skf_shape_distance_f32" in lib.skf_last_error()
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


def _front_end_want(A, B, S, center, cross=False):
    if center:
        A, B = [(ref.centered(p), q) for p, q in A], [(ref.centered(p), q) for p, q in B]
    return _want(A, B, S, cross)


def test_front_ends_through_the_real_tokenizers(tmp_path):
    from sketchformer_amd import align
    from sketchformer_amd.utils.tokenizer import GridTokenizer
    L = 100
    sketches = _synthetic_stroke3(8, seed=5)
    for tok in (GridTokenizer(resolution=16, max_seq_len=L), _dyadic_dict_tokenizer(tmp_path, 40, L)):
        a = np.stack([tok.encode(s) for s in sketches])                              # some rows truncated, some padded
        b = np.stack([tok.encode(s[::2]) for s in sketches[1:] + sketches[:1]])      # other sketches, thinned out
        b[3] = a[3]
        b[5] = tok.PAD                                                               # an empty sketch: the host's dummy row
        A, B = [ref.decoded_sketch(r, tok) for r in a], [ref.decoded_sketch(r, tok) for r in b]
        assert len(B[5][0]) == 1 and not B[5][0].any()
        for center in (False, True):
            want = _front_end_want(A, B, 4, center)
            parts = align.sketch_chamfer(a, b, kind="tokens", tokenizer=tok, center=center, return_parts=True)
            assert parts.is_cuda and tuple(parts.shape) == (8, 4)
            _assert_bits(parts, want, (type(tok).__name__, center))
            _assert_bits(align.sketch_hausdorff(a, b, kind="tokens", tokenizer=tok, center=center, return_parts=True), want, "parts")
            _assert_bits(align.sketch_chamfer(a, b, kind="tokens", tokenizer=tok, center=center), ref.chamfer(want), "chamfer")
            _assert_bits(align.sketch_hausdorff(a, b, kind="tokens", tokenizer=tok, center=center), ref.hausdorff(want), "hausdorff")
            assert want[3].max() < 1e-6 and want[[0, 1, 2]].min() > 1e-3       # the sketch against itself; against another
        cross = align.sketch_chamfer(a[:3], b, kind="tokens", tokenizer=tok, cross=True, samples_per_segment=2)
        _assert_bits(cross, ref.chamfer(_front_end_want(A[:3], B, 2, False, cross=True)), "cross chamfer")
        cross = align.sketch_hausdorff(a[:3], b, kind="tokens", tokenizer=tok, cross=True, samples_per_segment=2, center=True)
        _assert_bits(cross, ref.hausdorff(_front_end_want(A[:3], B, 2, True, cross=True)), "cross hausdorff, centred")


def test_front_ends_on_stroke5_and_ragged_stroke3():
    from sketchformer_amd import align
    import raster_reference as rr
    T = 65
    cases = rr.stroke5_cases(T, 31 + T)                             # dyadic offsets: their running sums are exact in any order
    s5 = np.stack([cases[k] for k in ("no_end", "end_middle", "end_first", "tie_lift_end")])
    other = s5[[1, 0, 3, 2]]
    host = lambda rows: [(p.astype(np.float32), q) for p, q in (rr.points_stroke5(r) for r in rows)]      # noqa: E731
    A, B = host(s5), host(other)
    assert min(len(p) for p, _ in A) == 0                           # an empty sketch is among them
    for center in (False, True):
        want = _front_end_want(A, B, 4, center)
        _assert_bits(align.sketch_chamfer(s5, other, kind="stroke5", center=center, return_parts=True), want, ("stroke5", center))
        _assert_bits(align.sketch_hausdorff(s5, other, kind="stroke5", center=center), ref.hausdorff(want), ("stroke5", center))
    # ragged stroke-3 lists
    rng = np.random.RandomState(4)
    walks = [rr.dyadic_walk(n, 50 + n) for n in (12, 1, 30)]
    pens = [(rng.uniform(size=len(w)) < 0.3).astype(np.float32) for w in walks]
    s3 = [np.c_[w, p].astype(np.float32) for w, p in zip(walks, pens)]
    A = [(np.cumsum(w, axis=0).astype(np.float32), p.astype(np.uint8)) for w, p in zip(walks, pens)]
    got = align.sketch_chamfer(s3, s3[::-1], kind="stroke3", return_parts=True, samples_per_segment=8)
    _assert_bits(got, _want(A, A[::-1], 8), "ragged stroke3")


def _stroke3_of(xy, pen):
    """absolute dyadic points + pen bytes -> stroke-3 rows (offsets from the origin; exact)"""
    return np.c_[np.diff(np.r_[np.zeros((1, 2), np.float32), xy], axis=0), pen].astype(np.float32)


def _dyadic_drawing(rng, n):
    xy = rng.randint(-64, 65, size=(n, 2)).astype(np.float32) / 64
    pen = (rng.uniform(size=n) < 0.25).astype(np.uint8)
    pen[-1] = 1
    pen[n // 2] = 1                                                  # at least two strokes
    return xy, pen


def test_stroke_order_is_invisible_to_chamfer_and_visible_to_dtw():
    from sketchformer_amd import align
    rng = np.random.RandomState(8)
    drawings = [_dyadic_drawing(rng, n) for n in (20, 64, 9)]
    moved = [ref.permute_strokes(xy, pen, order=np.roll(np.arange(int(pen.sum())), 1)) for xy, pen in drawings]
    a, b = [_stroke3_of(*d) for d in drawings], [_stroke3_of(*d) for d in moved]
    for center in (False, True):
        assert not align.sketch_chamfer(a, b, kind="stroke3", samples_per_segment=1, center=center, return_parts=True).cpu().numpy().any()
        assert not align.sketch_hausdorff(a, b, kind="stroke3", samples_per_segment=1, center=center).cpu().numpy().any()
    assert (align.sketch_dtw(a, b, kind="stroke3").cpu().numpy() > 0).all()
    # at S = 4 the interior samples of a segment need not lie on it to the last bit: tiny, and the same bits for either order
    third = [_stroke3_of(*_dyadic_drawing(rng, 30))] * 3
    assert torch.equal(align.sketch_chamfer(a, third, kind="stroke3", return_parts=True), align.sketch_chamfer(b, third, kind="stroke3", return_parts=True))


# ---------------------------------------------------------------- end to end
def test_metrics_on_a_tiny_synthetic_model(tmp_path):
    from sketchformer_amd import dataloaders, metrics, models
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=8,num_epochs=1,log_every=4",
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "sd")
    data = model.compute_predictions_on_validation_set()
    tok = dataset.tokenizer
    A, B = [ref.decoded_sketch(r, tok) for r in data[0]], [ref.decoded_sketch(r, tok) for r in data[2]]
    want = _want(A, B, 4)
    for name, fold in (("recon-chamfer", ref.chamfer), ("recon-hausdorff", ref.hausdorff)):
        metric = metrics.build_metric_by_name(name, model.hps)
        value = metric.compute(data)
        assert isinstance(value, float) and np.isfinite(value) and value >= 0
        # the metric's mean is float32 over at most 32 values: at most 32 roundings of 2^-24 relative each, of non-negative terms
        assert abs(value - float(fold(want).astype(np.float64).mean())) <= 32 * 2.0 ** -24 * value
        metric.computation_worker(data)                                            # the path a training run takes
        assert metric.last_value == value and metric.history == [value]
    # a perfect reconstruction: at S = 4 an interior sample lies on its own segment up to the rounding of a + t * e and of the
    # foot, a few ulp of the largest coordinate (8 allowed); a continuous reconstruction drops its start row
    perfect = (data[0], None, np.concatenate([data[0], np.zeros((len(data[0]), 1), data[0].dtype)], axis=1)) + tuple(data[3:])
    scale = max(float(np.abs(p).max()) for p, _ in A)
    assert 0.0 <= metrics.build_metric_by_name("recon-hausdorff", {}).compute(perfect) <= 8 * 2.0 ** -23 * scale
    import raster_reference as rr
    cases = rr.stroke5_cases(65, 96)
    s5 = np.stack([cases[k] for k in ("no_end", "end_middle", "end_first")])
    pred = np.concatenate([np.zeros((3, 1, 5), np.float32), s5[[1, 0, 2]]], axis=1)
    pred[:, 0, 2] = 1.0
    host = lambda rows: [(p.astype(np.float32), q) for p, q in (rr.points_stroke5(r) for r in rows)]      # noqa: E731
    want = ref.hausdorff(_want(host(s5), host(s5[[1, 0, 2]]), 4))
    value = metrics.build_metric_by_name("recon-hausdorff", {}).compute((s5, None, pred, None, None, None, None, None, True))
    assert value > 0 and abs(value - float(want.astype(np.float64).mean())) <= 32 * 2.0 ** -24 * value


@pytest.mark.parametrize("distance", ["chamfer", "hausdorff"])
def test_sequence_retrieval_experiment(tmp_path, distance):
    from sketchformer_amd import dataloaders, experiments, retrieval
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=4,n_samples=64"), None)
    model = types.SimpleNamespace(dataset=dataset)                  # the experiment uses model.dataset only
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    exp = Exp(Exp.parse_hparams("distance=%s,n_queries=8,n_gallery=32,top_k=5,gallery_block=12" % distance), "s0", str(tmp_path))
    out = np.load(exp.compute(model), allow_pickle=True)
    assert str(out["distance"]) == distance
    assert {"indices", "distances", "query_y", "gallery_y", "query_rows", "map_at_k", "precision_at_k", "recall_at_1", "per_class_ap",
            "class_names"} <= set(out.files)                         # the keys of retrieval.npz
    assert out["indices"].shape == (8, 5) and out["indices"].dtype == np.int32 and out["distances"].shape == (8, 5)
    tok = dataset.tokenizer
    gx, gy = dataset.get_all_data_from("test")
    gx, gy = gx[out["gallery_rows"]], gy.reshape(-1)[out["gallery_rows"]]
    qx = dataset.get_all_data_from("valid")[0][out["query_rows"]]
    Q, G = [ref.decoded_sketch(r, tok) for r in qx], [ref.decoded_sketch(r, tok) for r in gx]
    parts = _front_end_want(Q, G, 4, True, cross=True)              # centred, the default 4 samples per segment
    D = ref.chamfer(parts) if distance == "chamfer" else ref.hausdorff(parts)
    want = np.argsort(D, axis=1, kind="stable")[:, :5]
    assert np.array_equal(out["indices"], want)
    assert np.array_equal(_bits(out["distances"]), _bits(np.take_along_axis(D, want, axis=1)))
    scores = retrieval.retrieval_scores(want, out["query_y"], gy, exclude_self=False)
    assert float(out["map_at_k"]) == scores["map_at_k"] and float(out["recall_at_1"]) == scores["recall_at_1"]


def test_retrieval_ranks_a_stroke_permuted_copy_first_at_distance_zero(tmp_path):
    from sketchformer_amd import experiments
    rng = np.random.RandomState(31)
    T = 40

    def stroke5(xy, pen):
        rows = np.zeros((T, 5), np.float32)
        rows[:, 4] = 1.0                                             # end rows behind the drawing
        s3 = _stroke3_of(xy, pen)
        rows[:len(s3), :2], rows[:len(s3), 2], rows[:len(s3), 3], rows[:len(s3), 4] = s3[:, :2], 1 - s3[:, 2], s3[:, 2], 0
        return rows
    queries = [_dyadic_drawing(rng, n) for n in (12, 30, 7, 25, 18, 40, 9, 33)]
    gallery = [_dyadic_drawing(rng, rng.randint(5, T + 1)) for _ in range(32)]
    where = np.array([3, 30, 0, 17, 8, 21, 12, 26])                   # gallery row of the copy of query k
    for k, (xy, pen) in enumerate(queries):
        gallery[where[k]] = ref.permute_strokes(xy, pen, order=np.roll(np.arange(int(pen.sum())), 1))
        assert not np.array_equal(gallery[where[k]][0], xy)
    sets = {"valid": (np.stack([stroke5(*d) for d in queries]), np.arange(8) % 4),
            "test": (np.stack([stroke5(*d) for d in gallery]), np.arange(32) % 4)}
    dataset = types.SimpleNamespace(hps={"use_continuous_data": True}, get_all_data_from=lambda s: sets[s])
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    for distance in ("chamfer", "hausdorff"):
        hparams = "distance=%s,samples_per_segment=1,n_queries=8,n_gallery=32,top_k=5,gallery_block=12" % distance
        out = np.load(Exp(Exp.parse_hparams(hparams), distance, str(tmp_path)).compute(types.SimpleNamespace(dataset=dataset)), allow_pickle=True)
        assert str(out["distance"]) == distance
        assert np.array_equal(out["indices"][:, 0], where) and not out["distances"][:, 0].any() and (out["distances"][:, 1] > 0).all()
