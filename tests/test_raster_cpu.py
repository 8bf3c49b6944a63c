"""Host side of the sketch rasterizer: the float64 reference of tests/raster_reference.py against the project's host decoders and
against values worked out by hand, the float32 restatement of the raster formula against the float64 one, and the host helpers
and refusals of sketchformer_amd/raster.py.  Nothing here needs a device."""
import numpy as np
import pytest

import raster_reference as ref


def _raster():
    from sketchformer_amd import raster
    return raster


def _dict_tokenizer(tmp_path, centers):
    from sketchformer_amd.utils.tokenizer import Tokenizer
    path = str(tmp_path / "dict.npz")
    np.savez(path, cluster_centers=np.asarray(centers, np.float32), inertia=np.float64(0), n_iter=np.int64(1))
    return Tokenizer(path)


# ---------------------------------------------------------------- the reference decoders against the host decoders
@pytest.mark.parametrize("T", ref.POINT_LENGTHS)
def test_reference_decoders_match_the_host_decoders(tmp_path, T):
    _raster()                                            # (the feature these references restate must exist)
    from sketchformer_amd.metrics.samples import stroke5_to_stroke3
    from sketchformer_amd.utils.tokenizer import GridTokenizer
    K = 40
    centers = ref.dyadic_centers(K, 3)
    tok = _dict_tokenizer(tmp_path, centers)
    assert (tok.SEP, tok.SOS, tok.EOS) == (K + 1, K + 2, K + 3)
    for name, row in ref.token_cases(T, K, 11 + T).items():
        xy, pen = ref.points_dict(row, centers)
        if name == "out_of_vocab":
            with pytest.raises(IndexError):
                tok.decode_single([K + 100])             # the host raises; the definition skips
            continue
        host = tok.decode_single(row)
        if len(xy) == 0:
            assert np.array_equal(host, np.zeros((1, 3)))            # the host's dummy row; the definition says n_points = 0
            continue
        assert np.array_equal(np.cumsum(host[:, :2], axis=0), xy) and np.array_equal(host[:, 2], pen), name
    grid = GridTokenizer(resolution=10)
    R = grid.resolution
    assert (grid.SEP, grid.SOS, grid.EOS) == (R * R + 1, R * R + 2, R * R + 3)
    for name, row in ref.token_cases(T, R * R, 23 + T).items():
        xy, pen = ref.points_grid(row, R)
        host = grid.decode_single(row)                   # (this decoder skips an id outside the vocabulary too)
        if len(xy) == 0:
            assert np.array_equal(host, [[0.0, 0.0, 1.0]])
            continue
        np.testing.assert_allclose(np.cumsum(host[:, :2], axis=0), xy, rtol=0, atol=1e-12, err_msg=name)
        assert np.array_equal(host[:, 2], pen), name
    for name, rows in ref.stroke5_cases(T, 31 + T).items():
        xy, pen = ref.points_stroke5(rows)
        host = stroke5_to_stroke3(rows)
        assert len(host) == len(xy), name
        if len(xy):
            assert np.array_equal(np.cumsum(host[:, :2], axis=0), xy) and np.array_equal(host[:, 2], pen), name
    s3 = np.c_[ref.dyadic_walk(T, 5), (np.arange(T) % 4 == 3)]
    xy, pen = ref.points_stroke3(s3, T - T // 3)
    assert len(xy) == T - T // 3 and np.array_equal(xy, np.cumsum(s3[:T - T // 3, :2], axis=0)) and np.array_equal(pen, s3[:len(xy), 2])


def test_reference_row_cases_do_what_their_names_say():
    _raster()
    K, T = 40, 65
    centers = ref.dyadic_centers(K, 3)
    cases = ref.token_cases(T, K, 11 + T)
    n = {k: len(ref.points_dict(v, centers)[0]) for k, v in cases.items()}
    assert n["all_pad"] == 0 and n["no_sep"] == T and 0 < n["eos_middle"] <= T // 2
    assert ref.points_dict(cases["no_sep"], centers)[1].sum() == 0
    pen = ref.points_dict(cases["consecutive_seps"], centers)[1]
    assert 3 <= pen.sum() < (cases["consecutive_seps"] == K + 1).sum() - 2          # pairs lift one pen, the leading ones none
    assert n["out_of_vocab"] < T - 4
    s5 = ref.stroke5_cases(T, 31 + T)
    assert len(ref.points_stroke5(s5["no_end"])[0]) == T and len(ref.points_stroke5(s5["end_first"])[0]) == 0
    assert len(ref.points_stroke5(s5["end_middle"])[0]) == T // 2
    xy, pen = ref.points_stroke5(s5["tie_lift_end"])
    assert len(xy) == T and pen[-1] == 1


# ---------------------------------------------------------------- analytic values of the raster reference
UNIT_PIXELS = lambda H, W: (0.0, 0.0, float(W), float(H))        # noqa: E731  a frame that maps a point to itself at margin 0


def _draw(xy, pen, H, W, lw, frame=None, margin=0.0, dt=np.float64):
    return ref.rasterize(np.asarray(xy, np.float64), np.asarray(pen), UNIT_PIXELS(H, W) if frame is None else frame, H, W, lw, margin, dt)


@pytest.mark.parametrize("lw", [1.0, 1.5])
def test_horizontal_segment_through_pixel_centres(lw):
    _raster()
    H, W = 9, 16
    img = _draw([[2.5, 4.5], [12.5, 4.5]], [0, 0], H, W, lw)
    assert np.allclose(img[4, 2:13], 1.0, rtol=0, atol=1e-13)                 # on the line: d = 0 up to the rounding of t
    assert np.allclose(img[3, 2:13], 0.5 + lw / 2 - 1, atol=1e-15) and np.allclose(img[5, 2:13], 0.5 + lw / 2 - 1, atol=1e-15)
    assert (img[:2] == 0).all() and (img[7:] == 0).all()
    assert img[4, 1] == pytest.approx(min(1.0, max(0.0, 0.5 + lw / 2 - 1)))   # one pixel past the end: the cap is round


def test_dot_is_a_disc_and_pen_breaks_the_line():
    _raster()
    H = W = 15
    img = _draw([[7.5, 7.5]], [0], H, W, 5.0)
    yy, xx = np.mgrid[0:H, 0:W] + 0.5
    want = np.clip(3.0 - np.hypot(xx - 7.5, yy - 7.5), 0, 1)
    assert np.allclose(img, want, atol=1e-15) and img[7, 7] == 1 and img[7, 10] == 0 and img[7, 9] == 1
    joined = _draw([[2.5, 7.5], [12.5, 7.5]], [0, 0], H, W, 1.0)
    broken = _draw([[2.5, 7.5], [12.5, 7.5]], [1, 0], H, W, 1.0)
    assert joined[7, 7] == 1 and broken[7, 7] == 0 and broken[7, 2] == 1 and broken[7, 12] == 1
    assert np.array_equal(broken, np.maximum(_draw([[2.5, 7.5]], [0], H, W, 1.0), _draw([[12.5, 7.5]], [0], H, W, 1.0)))
    assert (_draw(np.zeros((0, 2)), np.zeros(0), H, W, 1.0) == 0).all()      # no points: blank


def test_frame_rules():
    _raster()
    # 'fit': the longer side of the box fills the canvas inside the margin, the box centre lands on the canvas centre
    s, cx, cy = ref.frame_scale((-1.0, 0.0, 3.0, 1.0), 64, 64, 2.0)
    assert (s, cx, cy) == (60.0 / 4.0, 1.0, 0.5)
    q = ref.to_pixels([[-1.0, 0.0], [3.0, 1.0], [1.0, 0.5]], (-1.0, 0.0, 3.0, 1.0), 64, 64, 2.0)
    assert np.array_equal(q, [[2.0, 24.5], [62.0, 39.5], [32.0, 32.0]])
    # 'unit' on a non-square canvas: the shorter side decides, y grows downwards
    s, cx, cy = ref.frame_scale((-1, -1, 1, 1), 24, 40, 2.0)
    assert (s, cx, cy) == (10.0, 0.0, 0.0)
    assert np.array_equal(ref.to_pixels([[-1, -1], [1, 1]], (-1, -1, 1, 1), 24, 40, 2.0), [[10.0, 2.0], [30.0, 22.0]])
    # a flat box: its zero side is left out of the min
    assert ref.frame_scale((0.0, 0.5, 2.0, 0.5), 24, 40, 2.0)[0] == 18.0
    assert ref.frame_scale((0.5, 0.0, 0.5, 2.0), 24, 40, 2.0)[0] == 10.0
    # a zero-size box: s = 0, everything at the canvas centre
    assert ref.frame_scale((0.5, 0.5, 0.5, 0.5), 24, 40, 2.0)[0] == 0.0
    assert np.array_equal(ref.to_pixels([[0.5, 0.5], [9.0, 9.0]], (0.5, 0.5, 0.5, 0.5), 24, 40, 2.0), [[20.0, 12.0], [20.0, 12.0]])
    img = ref.rasterize(np.array([[0.5, 0.5]]), np.zeros(1), (0.5, 0.5, 0.5, 0.5), 24, 40, 1.5)
    assert img[11:13, 19:21].min() > 0 and img.sum() == pytest.approx(4 * (1.25 - np.sqrt(0.5)) + 8 * max(0, 1.25 - np.sqrt(2.5)))
    assert np.allclose(ref.raster_bound(24, 40), 32 * 40 / 2 ** 24)


def test_float32_restatement_stays_below_a_thirtieth_of_the_bound():
    """The bound the device test applies per pixel is 32 * 2^-24 * max(H, W); the same formula in float32 numpy, in the kernel's
    arrangement (coordinates relative to the canvas centre), over the shapes of that test, stays below 1 / 30 of it."""
    _raster()
    worst = 0.0
    for (H, W), lengths in ref.RASTER_SHAPES:
        for xy, pen in ref.dyadic_sketches(lengths, seed=H):
            for lw in ref.LINE_WIDTHS:
                for frame in (ref.bounds(xy), ref.FIXED_FRAME):
                    a = ref.rasterize(xy, pen, frame, H, W, lw, 2.0, np.float64)
                    b = ref.rasterize(xy, pen, frame, H, W, lw, 2.0, np.float32, centred=True)
                    assert b.dtype == np.float32
                    if lw == 1.5:                        # centring the coordinates does not change the definition
                        assert np.abs(ref.rasterize(xy, pen, frame, H, W, lw, 2.0, np.float64, centred=True) - a).max() < 1e-12
                    err = np.abs(a - b).max() / ref.raster_bound(H, W)
                    print("%dx%d n=%d lw=%g: float32 error / bound = %.4f" % (H, W, len(xy), lw, err))
                    worst = max(worst, err)
    assert worst < 1.0 / 30.0, worst


# ---------------------------------------------------------------- soft IoU
def test_soft_iou_edge_cases():
    raster = _raster()
    rng = np.random.RandomState(0)
    a = rng.rand(8, 8)
    assert ref.soft_iou(a, a) == 1.0
    b, c = np.zeros((8, 8)), np.zeros((8, 8))
    b[:4], c[4:] = a[:4], a[4:]
    assert ref.soft_iou(b, c) == 0.0 and ref.soft_iou(np.zeros((8, 8)), np.zeros((8, 8))) == 1.0
    assert ref.soft_iou(a, 0.5 * a) == pytest.approx(0.5)
    sums = np.array([[3.0, 3.0], [0.0, 2.0], [0.0, 0.0], [1.0, 4.0]], dtype=np.float32)
    assert np.array_equal(raster.iou_from_sums(sums), np.array([1.0, 0.0, 1.0, 0.25], dtype=np.float32))
    import torch
    assert torch.equal(raster.iou_from_sums(torch.from_numpy(sums)), torch.tensor([1.0, 0.0, 1.0, 0.25]))


# ---------------------------------------------------------------- host helpers
def test_to_uint8_contact_sheet_and_png_round_trip(tmp_path):
    raster = _raster()
    cov = np.array([[[0.0, 1.0], [0.5, 0.25]]])
    u8 = raster.to_uint8(cov)
    assert u8.dtype == np.uint8 and np.array_equal(u8, [[[255, 0], [128, 191]]])       # dark ink on white paper
    assert np.array_equal(raster.to_uint8(np.array([[[-1.0, 2.0, np.nan]]])), [[[255, 0, 255]]])
    imgs = (np.arange(5 * 2 * 3).reshape(5, 2, 3) % 200).astype(np.uint8)
    sheet = raster.contact_sheet(imgs, cols=3, pad=1)
    assert sheet.shape == (2 * 3 + 1, 3 * 4 + 1) and sheet.dtype == np.uint8
    for k in range(5):
        r, c = divmod(k, 3)
        assert np.array_equal(sheet[1 + 3 * r:3 + 3 * r, 1 + 4 * c:4 + 4 * c], imgs[k])
    assert (sheet[4:6, 9:12] == 255).all() and (sheet[0] == 255).all() and (sheet[:, 0] == 255).all()
    assert np.array_equal(raster.contact_sheet(imgs[:1], cols=6, pad=0), np.c_[imgs[0], np.full((2, 15), 255, np.uint8)])
    inter = raster.interlace(imgs[:2], imgs[2:4])
    assert np.array_equal(inter, imgs[[0, 2, 1, 3]])
    path = raster.save_png(str(tmp_path / "sheet.png"), sheet)
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    try:
        from matplotlib import pyplot as plt
        back = plt.imread(path)
        back = np.rint(back[..., 0] * 255).astype(np.uint8) if back.ndim == 3 else np.rint(back * 255).astype(np.uint8)
    except ImportError:
        from PIL import Image
        back = np.asarray(Image.open(path).convert("L"))
    assert np.array_equal(back, sheet)
    a, lens = raster.pack_stroke3([np.zeros((0, 3)), np.ones((4, 3)), np.ones((2, 3))])
    assert a.shape == (3, 4, 3) and a.dtype == np.float32 and lens.tolist() == [0, 4, 2] and a[2, 2:].sum() == 0


def test_python_level_refusals(tmp_path):
    raster = _raster()
    import torch
    from sketchformer_amd import _lib, ops
    s = np.zeros((2, 5, 3), np.float32)
    with pytest.raises(ValueError, match="kind"):
        raster.render(s, kind="svg")
    with pytest.raises(ValueError, match="tokenizer"):
        raster.render(np.zeros((2, 5), np.int64), kind="tokens")
    for bad in (dict(size=(0, 8)), dict(line_width=0.0), dict(line_width=-1.0), dict(margin=-0.5), dict(size=(8, 64), margin=4.0),
                dict(frame="stretch")):
        with pytest.raises(ValueError):
            raster.render(s, **bad)
    with pytest.raises(ValueError):
        raster.save_png(str(tmp_path / "x.png"), np.zeros((4, 4)))                      # not uint8
    with pytest.raises(ValueError):
        raster.contact_sheet(np.zeros((0, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        raster.pack_stroke3([])
    # no CPU path: host tensors are refused by the wrappers
    t = torch.zeros(2, 5, 3)
    with pytest.raises(_lib.SkfError):
        ops.sketch_points(t, "stroke3", lengths=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_lib.SkfError):
        ops.rasterize(torch.zeros(2, 5, 2), torch.zeros(2, 5, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4), (8, 8))
    with pytest.raises(_lib.SkfError):
        raster.soft_iou(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8))
    with pytest.raises(ValueError):
        ops.sketch_points(t, "polyline")
    # the metric and the experiment are registered by name
    from sketchformer_amd import experiments, metrics
    assert metrics.metrics_by_name["recon-raster-iou"].input_type == "predictions_on_validation_set"
    assert experiments.get_experiment_by_name("rendered-reconstructions").requires_model
