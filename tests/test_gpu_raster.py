"""The sketch rasterizer on the device (skf_raster.hip) against the float64 definitions of tests/raster_reference.py.

Points: counts, pens and grid positions are exact; positions summed from offsets are exact for dyadic offsets (every partial sum
is representable) and within n * 2^-24 * max|p| for random float32 ones.  Raster: every pixel within 32 * 2^-24 * max(H, W) of the
float64 reference - coverage is 1-Lipschitz in the pixel-space coordinates, and the bound allows 32 roundings at the magnitude of
the largest pixel coordinate (tests/test_raster_cpu.py holds a float32 restatement of the formula below 1 / 30 of it).  No case
is left out: coverage is continuous in every input."""
import os

import numpy as np
import pytest
import torch

import raster_reference as ref

pytestmark = pytest.mark.gpu


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_points(got, want, exact, label):
    """got: (xy, pen, n, bounds) device tensors; want: [(xy float64, pen)] per sketch"""
    xy, pen, n, bnd = (t.cpu().numpy() for t in got)
    assert xy.dtype == np.float32 and pen.dtype == np.uint8 and n.dtype == np.int32 and bnd.dtype == np.float32
    for i, (wxy, wpen) in enumerate(want):
        k = len(wxy)
        assert n[i] == k, (label, i, n[i], k)
        assert np.array_equal(pen[i, :k], wpen), (label, i)
        assert not xy[i, k:].any() and not pen[i, k:].any(), (label, i)          # the rows behind the sketch are zero
        if k == 0:
            assert not bnd[i].any()
            continue
        if exact:
            assert np.array_equal(xy[i, :k].astype(np.float64), wxy.astype(np.float32).astype(np.float64)), (label, i)
        else:
            tol = k * 2.0 ** -24 * np.abs(wxy).max()
            err = np.abs(xy[i, :k].astype(np.float64) - wxy).max()
            print("%s[%d]: n = %d, position error %.3g (bound %.3g)" % (label, i, k, err, tol))
            assert err <= tol, (label, i, err, tol)
        assert np.array_equal(bnd[i], np.r_[xy[i, :k].min(0), xy[i, :k].max(0)]), (label, i)


def _batches(cases):
    names = sorted(cases)
    for at in range(0, len(names), 3):
        pick = (names[at:at + 3] + names)[:3]                                    # B = 3
        yield pick, [cases[k] for k in pick]


# ---------------------------------------------------------------- points
@pytest.mark.parametrize("T", ref.POINT_LENGTHS)
@pytest.mark.parametrize("kind", ["stroke3", "stroke5", "dict_tokens", "grid_tokens"])
def test_points_are_exact_on_dyadic_inputs(kind, T):
    from sketchformer_amd import ops
    if kind == "stroke3":
        rows = np.stack([np.c_[ref.dyadic_walk(T, 50 + k), np.arange(T) % (k + 3) == 2] for k in range(3)]).astype(np.float32)
        lengths = np.array([T, T - T // 3, 0], dtype=np.int32)
        got = ops.sketch_points(_d(rows), "stroke3", lengths=_d(lengths))
        _check_points(got, [ref.points_stroke3(rows[i], lengths[i]) for i in range(3)], True, "stroke3 T=%d" % T)
        return
    if kind == "stroke5":
        for names, rows in _batches(ref.stroke5_cases(T, 31 + T)):
            got = ops.sketch_points(_d(np.stack(rows)), "stroke5")
            _check_points(got, [ref.points_stroke5(r) for r in rows], True, "stroke5 T=%d %s" % (T, names))
        return
    if kind == "dict_tokens":
        K = 40
        centers = ref.dyadic_centers(K, 3)
        for names, rows in _batches(ref.token_cases(T, K, 11 + T)):
            got = ops.sketch_points(_d(np.stack(rows)), "dict_tokens", centers=_d(centers))
            _check_points(got, [ref.points_dict(r, centers) for r in rows], True, "dict T=%d %s" % (T, names))
        return
    for R in (10, 100):
        for names, rows in _batches(ref.token_cases(T, R * R, 23 + T)):
            got = ops.sketch_points(_d(np.stack(rows)), "grid_tokens", resolution=R)
            _check_points(got, [ref.points_grid(r, R) for r in rows], True, "grid R=%d T=%d %s" % (R, T, names))


@pytest.mark.parametrize("T", ref.POINT_LENGTHS)
def test_points_of_random_float32_offsets_stay_within_the_summation_bound(T):
    from sketchformer_amd import ops
    rng = np.random.RandomState(T)
    rows = np.concatenate([rng.randn(3, T, 2) * [[[0.05]], [[1.0]], [[30.0]]], rng.rand(3, T, 1) < 0.2], axis=2).astype(np.float32)
    lengths = np.full(3, T, dtype=np.int32)
    got = ops.sketch_points(_d(rows), "stroke3", lengths=_d(lengths))
    _check_points(got, [ref.points_stroke3(rows[i], T) for i in range(3)], False, "stroke3 random T=%d" % T)
    s5 = np.zeros((3, T, 5), dtype=np.float32)
    s5[:, :, :2] = rows[:, :, :2]
    s5[:, :, 2:] = rng.rand(3, T, 3) * [1.0, 0.6, 0.0]                           # no end row
    got = ops.sketch_points(_d(s5), "stroke5")
    _check_points(got, [ref.points_stroke5(r) for r in s5], False, "stroke5 random T=%d" % T)
    K = 1000
    centers = (rng.randn(K, 2) * 0.1).astype(np.float32)
    cases = ref.token_cases(T, K, 5 + T)
    tok = np.stack([cases["plain"], cases["no_sep"], cases["consecutive_seps"]])
    got = ops.sketch_points(_d(tok), "dict_tokens", centers=_d(centers))
    _check_points(got, [ref.points_dict(r, centers) for r in tok], False, "dict random T=%d" % T)


def test_points_read_the_first_T_columns_of_wider_token_rows():
    from sketchformer_amd import ops
    K, T, ld = 40, 65, 80
    centers = ref.dyadic_centers(K, 3)
    wide = np.full((3, ld), 7, dtype=np.int64)                                    # ids behind column T must not be read as points
    rows = [ref.token_cases(T, K, 11 + T)[k] for k in ("plain", "no_sep", "all_pad")]
    wide[:, :T] = np.stack(rows)
    got = ops.sketch_points(_d(wide), "dict_tokens", centers=_d(centers), T=T)
    assert got[0].shape == (3, T, 2)
    _check_points(got, [ref.points_dict(r, centers) for r in rows], True, "wide rows")
    view = _d(np.concatenate([wide, wide], axis=1))[:, :T]                        # a strided view: ld = 160
    _check_points(ops.sketch_points(view, "dict_tokens", centers=_d(centers)), [ref.points_dict(r, centers) for r in rows], True, "view")


# ---------------------------------------------------------------- raster against the float64 reference
def _rasterize(sketches, frames, H, W, lw, margin=2.0):
    from sketchformer_amd import ops
    xy, pen, n, _ = ref.pack_points(sketches)
    return ops.rasterize(_d(xy), _d(pen), _d(n), _d(np.asarray(frames, np.float32)), (H, W), lw, margin).cpu().numpy()


def _check_images(got, sketches, frames, H, W, lw, label, margin=2.0):
    assert got.shape == (len(sketches), H, W) and got.dtype == np.float32
    bound = ref.raster_bound(H, W)
    for i, (xy, pen) in enumerate(sketches):
        want = ref.rasterize(xy, pen, np.asarray(frames[i], np.float32).astype(np.float64), H, W, lw, margin)
        err = np.abs(got[i].astype(np.float64) - want).max()
        print("%s[%d]: n = %d, ink %.4f, error / bound = %.4f" % (label, i, len(xy), want.mean(), err / bound))
        assert err <= bound, (label, i, err, bound)
        assert got[i].min() >= 0.0 and got[i].max() <= 1.0


@pytest.mark.parametrize("frame", ["fit", "fixed"])
@pytest.mark.parametrize("lw", ref.LINE_WIDTHS)
@pytest.mark.parametrize("shape", ref.RASTER_SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_raster_matches_the_float64_reference(shape, lw, frame):
    (H, W), lengths = shape
    sketches = ref.dyadic_sketches(lengths, seed=H)
    frames = [ref.bounds(xy) if frame == "fit" else ref.FIXED_FRAME for xy, _ in sketches]
    if frame == "fixed":                                                          # part of the longer sketches lies outside the canvas
        q = ref.to_pixels(sketches[-1][0], ref.FIXED_FRAME, H, W, 2.0)
        assert (q.min() < -1.0 or q[:, 0].max() > W + 1.0 or q[:, 1].max() > H + 1.0) and ((q >= 0).all(1) & (q[:, 0] <= W) & (q[:, 1] <= H)).any()
    got = _rasterize(sketches, frames, H, W, lw)
    _check_images(got, sketches, frames, H, W, lw, "%dx%d lw=%g %s" % (H, W, lw, frame))


def test_render_fit_uses_the_device_bounds_and_unit_the_unit_box():
    """raster.render end to end from ragged stroke-3 offsets: points, bounds, frames and images in one go"""
    from sketchformer_amd import raster
    H, W = 24, 40
    sketches = ref.dyadic_sketches((7, 65, 33), seed=77)
    s3 = [np.c_[np.diff(np.r_[np.zeros((1, 2)), xy], axis=0), pen] for xy, pen in sketches]
    img, frames = raster.render(s3, kind="stroke3", size=(H, W), frame="fit", return_frames=True)
    frames = frames.cpu().numpy()
    assert np.array_equal(frames, np.stack([ref.bounds(xy) for xy, _ in sketches]).astype(np.float32))
    _check_images(img.cpu().numpy(), sketches, frames, H, W, 1.5, "render fit")
    unit = raster.render(s3, kind="stroke3", size=(H, W), frame="unit", line_width=1.0)
    _check_images(unit.cpu().numpy(), sketches, [raster.UNIT_FRAME] * 3, H, W, 1.0, "render unit")
    again = raster.render(s3, kind="stroke3", size=(H, W), frame=frames)
    assert torch.equal(again, img)


# ---------------------------------------------------------------- named cases
PIXEL_FRAME = lambda H, W: (0.0, 0.0, float(W), float(H))        # noqa: E731  with margin 0 a point is its own pixel position


def test_one_diagonal_crosses_every_tile_of_the_large_canvas():
    H = W = 256
    sk = [(np.array([[-1.0, -1.0], [1.0, 1.0]]), np.zeros(2, np.uint8)), (np.array([[-1.0, 1.0], [1.0, -1.0]]), np.zeros(2, np.uint8))]
    frames = [(-1.0, -1.0, 1.0, 1.0)] * 2
    got = _rasterize(sk, frames, H, W, 1.5)
    _check_images(got, sk, frames, H, W, 1.5, "diagonal")
    for t in range(8):                                                            # the tiles on the diagonal carry ink, the far corners none
        assert got[0, 32 * t:32 * t + 32, 32 * t:32 * t + 32].max() == 1.0
        assert got[1, 32 * t:32 * t + 32, 224 - 32 * t:256 - 32 * t].max() == 1.0
    assert got[0, :64, 192:].max() == 0.0 and got[1, :64, :64].max() == 0.0


def test_wide_line_reaches_into_the_neighbouring_tile():
    """line width 9: the centre line lies in tile row 1 (y = 35), its ink reaches rows 30 and 31 of tile row 0 - only a culling box
    grown by line_width / 2 + 0.5 keeps the segment for that tile; the same for columns"""
    H = W = 64
    sk = [(np.array([[2.0, 35.0], [62.0, 35.0]]), np.zeros(2, np.uint8)), (np.array([[35.0, 2.0], [35.0, 62.0]]), np.zeros(2, np.uint8)),
          (np.array([[2.0, 36.5], [62.0, 36.5]]), np.zeros(2, np.uint8))]
    frames = [PIXEL_FRAME(H, W)] * 3
    got = _rasterize(sk, frames, H, W, 9.0, margin=0.0)
    _check_images(got, sk, frames, H, W, 9.0, "wide line", margin=0.0)
    assert (got[0, 31, 4:60] == 1.0).all() and (got[0, 30, 4:60] == 0.5).all() and (got[0, 29] == 0.0).all()
    assert (got[1, 4:60, 31] == 1.0).all() and (got[1, 4:60, 30] == 0.5).all() and (got[1, :, 29] == 0.0).all()
    assert (got[2, 31, 4:60] == 0.0).all() and (got[2, 32, 4:60] == 1.0).all()  # d = 5 at row 31: exactly at the edge of the ink


def test_degenerate_sketches():
    from sketchformer_amd import ops
    H, W = 24, 40
    # a segment wholly outside a fixed frame: blank
    sk = [(np.array([[3.0, 3.0], [4.0, 3.5]]), np.zeros(2, np.uint8))]
    assert not _rasterize(sk, [(-1.0, -1.0, 1.0, 1.0)], H, W, 9.0).any()
    # n_points = 0 and 1
    xy = np.zeros((2, 5, 2), np.float32)
    xy[:, 0] = (0.25, -0.5)
    xy[:, 1:] = 0.75                                                              # rows behind n_points must not be drawn
    frames = np.array([[-1.0, -1.0, 1.0, 1.0]] * 2, np.float32)
    got = ops.rasterize(_d(xy), _d(np.zeros((2, 5), np.uint8)), _d(np.array([0, 1], np.int32)), _d(frames), (H, W), 1.5).cpu().numpy()
    assert not got[0].any()
    _check_images(got[1:], [(np.array([[0.25, -0.5]]), np.zeros(1, np.uint8))], frames[1:], H, W, 1.5, "one point")
    assert got[1].max() > 0.5 and (got[1] > 0).sum() <= 9
    # all pens lifted: dots only
    dots = [(xy_, np.ones(len(xy_), np.uint8)) for xy_, _ in ref.dyadic_sketches((33,), seed=5)]
    frames = [ref.bounds(dots[0][0])]
    got = _rasterize(dots, frames, H, W, 1.5)
    _check_images(got, dots, frames, H, W, 1.5, "dots")
    lines = _rasterize([(dots[0][0], np.zeros(33, np.uint8))], frames, H, W, 1.5)
    assert (got <= lines + 1e-4).all() and got.sum() < lines.sum()              # every dot lies on the polyline
    # coinciding points: a zero-size box, s = 0, a dot at the canvas centre
    same = [(np.full((4, 2), 0.375), np.zeros(4, np.uint8))]
    got = _rasterize(same, [ref.bounds(same[0][0])], H, W, 1.5)
    _check_images(got, same, [ref.bounds(same[0][0])], H, W, 1.5, "coinciding")
    assert got[0, 11:13, 19:21].min() > 0.5 and got[0].sum() == pytest.approx(4 * (1.25 - np.sqrt(0.5)), abs=1e-4)


def test_refusals():
    from sketchformer_amd import _lib, ops
    xy, pen, n, frames = _d(np.zeros((1, 4, 2), np.float32)), _d(np.zeros((1, 4), np.uint8)), _d(np.ones(1, np.int32)), _d(np.zeros((1, 4), np.float32))
    for size, lw, margin in (((0, 8), 1.5, 0.0), ((8, 0), 1.5, 0.0), ((8, 8), 0.0, 1.0), ((8, 8), -1.0, 1.0), ((8, 8), 1.5, -0.5),
                             ((8, 8), 1.5, 4.0), ((8, 64), 1.5, 4.5)):
        with pytest.raises(_lib.SkfError, match="rc=-1"):
            ops.rasterize(xy, pen, n, frames, size, lw, margin)
    assert ops.rasterize(xy, pen, n, frames, (8, 64), 1.5, 3.5).shape == (1, 8, 64)
    tok = _d(np.zeros((2, 8), np.int64))
    with pytest.raises(_lib.SkfError, match="rc=-1"):
        ops.sketch_points(tok, "grid_tokens", resolution=7)                      # the grid tokenizer's resolution is even
    with pytest.raises(TypeError):
        ops.sketch_points(tok, "dict_tokens")                                     # no centres
    with pytest.raises(TypeError):
        ops.sketch_points(_d(np.zeros((2, 8, 3), np.float32)), "stroke3")         # no lengths
    with pytest.raises(ValueError):
        ops.raster_overlap(_d(np.zeros((2, 8, 8), np.float32)), _d(np.zeros((2, 8, 4), np.float32)))


# ---------------------------------------------------------------- independence and reproducibility
def test_a_sketch_does_not_depend_on_its_batch_and_runs_repeat_bit_for_bit():
    from sketchformer_amd import ops
    H, W = 64, 64
    sketches = ref.dyadic_sketches((2, 64, 300), seed=H)
    xy, pen, n, bnd = (_d(a) for a in ref.pack_points(sketches))
    a = ops.rasterize(xy, pen, n, bnd, (H, W), 1.5)
    b = ops.rasterize(xy, pen, n, bnd, (H, W), 1.5)
    assert torch.equal(a, b)
    for i in range(3):
        alone = ops.rasterize(xy[i:i + 1].contiguous(), pen[i:i + 1].contiguous(), n[i:i + 1].contiguous(), bnd[i:i + 1].contiguous(), (H, W), 1.5)
        assert torch.equal(alone[0], a[i]), i
    order = torch.tensor([2, 0, 1], device=xy.device)
    c = ops.rasterize(xy[order].contiguous(), pen[order].contiguous(), n[order].contiguous(), bnd[order].contiguous(), (H, W), 1.5)
    assert torch.equal(c, a[order])
    # the same for the points
    rows = np.stack([np.c_[ref.dyadic_walk(300, 50 + k), np.arange(300) % 5 == 2] for k in range(3)]).astype(np.float32)
    lens = _d(np.array([300, 200, 65], np.int32))
    p = ops.sketch_points(_d(rows), "stroke3", lengths=lens)
    q = ops.sketch_points(_d(rows), "stroke3", lengths=lens)
    assert all(torch.equal(u, v) for u, v in zip(p, q))
    one = ops.sketch_points(_d(rows[1:2]), "stroke3", lengths=lens[1:2].contiguous())
    assert all(torch.equal(u[0], v[1]) for u, v in zip(one, p))


# ---------------------------------------------------------------- overlap
@pytest.mark.parametrize("shape", [(24, 40), (64, 64), (256, 256), (5, 7)])
def test_overlap_sums_and_iou(shape):
    from sketchformer_amd import ops, raster
    H, W = shape
    rng = np.random.RandomState(H)
    a = (rng.rand(3, H, W) * (rng.rand(3, H, W) < 0.3)).astype(np.float32)
    b = (rng.rand(3, H, W) * (rng.rand(3, H, W) < 0.3)).astype(np.float32)
    b[2] = 0
    got = ops.raster_overlap(_d(a), _d(b)).cpu().numpy()
    assert got.shape == (3, 2) and got.dtype == np.float32
    for i in range(3):
        want = ref.overlap(a[i], b[i])
        assert np.all(np.abs(got[i] - want) <= H * W * 2.0 ** -24 * np.abs(want)), (i, got[i], want)
    assert torch.equal(ops.raster_overlap(_d(a), _d(b)), ops.raster_overlap(_d(a), _d(b)))
    iou = raster.soft_iou(_d(a), _d(b)).cpu().numpy()
    for i in range(3):
        assert iou[i] == pytest.approx(ref.soft_iou(a[i], b[i]), rel=2 * H * W * 2.0 ** -24, abs=0)
    assert iou[2] == 0.0
    same = ops.raster_overlap(_d(a), _d(a)).cpu().numpy()
    assert np.array_equal(same[:, 0], same[:, 1])
    assert np.array_equal(raster.soft_iou(_d(a), _d(a)).cpu().numpy(), np.ones(3, np.float32))           # exactly 1
    blank = _d(np.zeros((3, H, W), np.float32))
    assert np.array_equal(raster.soft_iou(blank, blank).cpu().numpy(), np.ones(3, np.float32))            # both blank: 1


# ---------------------------------------------------------------- end to end
def _small_model(tmp_path, batch, continuous=False):
    from sketchformer_amd import dataloaders, models
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams("max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"), None)
    model = Model(Model.parse_hparams(base="batch_size=%d,num_epochs=1,log_every=4" % batch,
                                      specific="num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"),
                  dataset, str(tmp_path), "rr")
    return model, dataset


def _reference_pair_iou(tok, x, recon, size, lw):
    out = []
    for a, b in zip(x, recon):
        pa, pb = (np.asarray(tok.decode_single(s), np.float64) for s in (a, b))
        xa, xb = np.cumsum(pa[:, :2], axis=0), np.cumsum(pb[:, :2], axis=0)
        frame = ref.bounds(xa)
        out.append(ref.soft_iou(ref.rasterize(xa, pa[:, 2] == 1, frame, size, size, lw), ref.rasterize(xb, pb[:, 2] == 1, frame, size, size, lw)))
    return np.array(out)


def test_rendered_reconstructions_experiment_and_metric(tmp_path):
    from sketchformer_amd import experiments, metrics, raster
    model, dataset = _small_model(tmp_path, 8)
    tok = dataset.tokenizer
    Exp = experiments.get_experiment_by_name("rendered-reconstructions")
    assert dict(Exp.default_hparams().values())["n_sketches"] == 32 and dict(Exp.default_hparams().values())["size"] == 128
    exp = Exp(Exp.parse_hparams("n_sketches=10,size=48,line_width=1.5"), "r0", str(tmp_path))
    path = exp.compute(model)
    out = np.load(path, allow_pickle=True)
    assert {"originals", "reconstructions", "iou", "mean_iou", "inputs", "recon"} <= set(out.files)
    assert out["originals"].shape == (10, 48, 48) and out["originals"].dtype == np.uint8
    assert out["reconstructions"].shape == (10, 48, 48) and out["reconstructions"].dtype == np.uint8
    assert out["originals"].max() == 255 and out["originals"].min() == 0            # dark ink on white paper
    assert out["iou"].shape == (10,) and float(out["mean_iou"]) == pytest.approx(out["iou"].astype(np.float64).mean())
    png = os.path.join(os.path.dirname(path), str(out["plot"]))
    assert os.path.isfile(png) and open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    x, _ = dataset.get_n_samples_from("valid", 10, shuffled=True, seeded=True)
    assert np.array_equal(out["inputs"], x) and out["recon"].shape == (10, 25)
    want = _reference_pair_iou(tok, out["inputs"], out["recon"], 48, 1.5)
    err = np.abs(out["iou"] - want).max()
    print("experiment iou %s, reference %s, largest difference %.3g (bound %.3g)" % (out["iou"], want, err, ref.raster_bound(48, 48)))
    assert err <= ref.raster_bound(48, 48)
    assert ((out["iou"] >= 0) & (out["iou"] <= 1)).all()
    # a sketch against itself: exactly 1 for every sketch
    a, b, iou = raster.render_pair_iou(x, x, kind="tokens", tokenizer=tok, size=(48, 48))
    assert torch.equal(a, b) and np.array_equal(iou.cpu().numpy(), np.ones(10, np.float32))
    # the metric
    metric = metrics.build_metric_by_name("recon-raster-iou", model.hps)
    data = model.compute_predictions_on_validation_set()
    value = metric.compute(data)
    assert isinstance(value, float) and np.isfinite(value) and 0.0 <= value <= 1.0
    want = _reference_pair_iou(tok, data[0], data[2], 64, 1.5).mean()
    assert abs(value - want) <= ref.raster_bound(64, 64)
    metric.computation_worker(data)                                              # the path a training run takes
    assert metric.last_value == value and metric.history == [value]


def test_pair_iou_and_metric_on_continuous_and_tokenizer_inputs(tmp_path):
    """render_pair_iou(x, x) is exactly 1 through every decoder, and the metric drops the start row of a continuous reconstruction"""
    from sketchformer_amd import metrics, raster
    from sketchformer_amd.utils.tokenizer import GridTokenizer, Tokenizer
    T = 65
    s5 = np.stack([ref.stroke5_cases(T, 31 + T)[k] for k in ("no_end", "end_middle", "end_first")])
    _, _, iou = raster.render_pair_iou(s5, s5, kind="stroke5")
    assert np.array_equal(iou.cpu().numpy(), np.ones(3, np.float32))
    grid = GridTokenizer(resolution=10)
    cases = ref.token_cases(T, 100, 23 + T)
    tok_rows = np.stack([cases[k] for k in ("plain", "eos_middle", "all_pad")])
    a, _, iou = raster.render_pair_iou(tok_rows, tok_rows, kind="tokens", tokenizer=grid, size=(24, 40))
    assert np.array_equal(iou.cpu().numpy(), np.ones(3, np.float32)) and not a[2].any() and a[0].max() == 1.0
    sk = [ref.points_grid(r, 10) for r in tok_rows]
    _check_images(a.cpu().numpy(), sk, [ref.bounds(xy) for xy, _ in sk], 24, 40, 1.5, "grid tokens")
    path = str(tmp_path / "dict.npz")
    centers = ref.dyadic_centers(40, 3)
    np.savez(path, cluster_centers=centers, inertia=np.float64(0), n_iter=np.int64(1))
    cases = ref.token_cases(T, 40, 11 + T)
    tok_rows = np.stack([cases[k] for k in ("plain", "consecutive_seps", "no_sep")])
    a, _, iou = raster.render_pair_iou(tok_rows, tok_rows, kind="tokens", tokenizer=Tokenizer(path), size=(24, 40))
    assert np.array_equal(iou.cpu().numpy(), np.ones(3, np.float32))
    sk = [ref.points_dict(r, centers) for r in tok_rows]
    _check_images(a.cpu().numpy(), sk, [ref.bounds(xy) for xy, _ in sk], 24, 40, 1.5, "dict tokens")
    # the metric on continuous data: pred_x carries the start row, the originals do not
    metric = metrics.build_metric_by_name("recon-raster-iou", {})
    pred = np.concatenate([np.zeros((3, 1, 5), np.float32), s5], axis=1)
    pred[:, 0, 2] = 1.0
    data = (s5, None, pred, None, None, None, None, None, True)
    assert metric.compute(data) == 1.0
    shifted = np.concatenate([s5, np.zeros((3, 1, 5), np.float32)], axis=1)       # the start row NOT dropped would look like this
    assert metric.compute((s5, None, shifted, None, None, None, None, None, True)) < 1.0
