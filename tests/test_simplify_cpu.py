"""Stroke simplification, the parts that need no GPU: the host restatement against the same rule in Python integers, the named
fixtures that give tests/test_gpu_simplify.py its teeth (asserted here so that the GPU tests cannot pass by accident), the host
helpers, and the chunk script against what the reference's script wrote (tests/golden/prepare_quickdraw/, recorded by
tools/record_prepare_quickdraw_golden.py)."""
import os

import numpy as np
import pytest

import simplify_reference as ref
from sketchformer_amd import simplify

ROOT, GOLDEN = ref.ROOT, ref.GOLDEN


@pytest.mark.parametrize("epsilon", [1.0, 2.0])
def test_the_restatement_is_exact_on_integer_strokes(epsilon):
    pool = ref.int_pool()
    assert {len(l) for l in pool} >= set(ref.STROKE_LENGTHS)
    for line in pool:
        assert np.array_equal(ref.rdp_mask(line, epsilon), ref.rdp_mask_exact(line, epsilon)), len(line)


def test_among_equal_distances_the_lowest_index_wins():
    points, epsilon, want = ref.TENT
    assert ref.rdp_mask(points, epsilon).tolist() == want
    assert ref.rdp_mask_exact(points, "9/2").tolist() == want
    assert ref.rdp_mask(points, epsilon, last_max_wins=True).tolist() != want


def test_a_closed_segment_measures_the_distance_to_its_point():
    points, epsilon, want = ref.SQUARE
    assert ref.rdp_mask(points, epsilon).tolist() == want


def test_the_comparison_is_strict():
    points, epsilon, want = ref.COLLINEAR
    assert ref.rdp_mask(points, epsilon).tolist() == want


@pytest.mark.parametrize("n", ref.ZIGZAG_LENGTHS)
def test_the_zigzag_keeps_everything_one_level_a_point(n):
    keep, depth = ref.rdp_mask(ref.zigzag(n), 2.0, return_depth=True)
    assert keep.tolist() == [1] * n and depth == n - 1


def test_short_polylines_keep_everything():
    for n in (0, 1, 2):
        keep, depth = ref.rdp_mask(ref.zigzag(n), 1e9, return_depth=True)
        assert keep.tolist() == [1] * n and depth == (1 if n == 2 else 0)
    assert ref.rdp_mask(ref.zigzag(9), 1e9).tolist() == [1] + [0] * 7 + [1]


def test_smooth_strokes_lose_most_of_their_interior():
    """A kernel that keeps everything must fail: at epsilon 2 the pool's smooth strokes drop more than half of their interior
    points (this generator: 2610 of 3103), the uniform-float strokes next to nothing."""
    pool = ref.int_pool()
    interior = sum(max(len(l) - 2, 0) for l in pool)
    dropped = sum(int((ref.rdp_mask(l, 2.0) == 0).sum()) for l in pool)
    assert interior > 3000 and 2 * dropped > interior, (dropped, interior)
    floats = ref.float_pool()
    assert sum(int((ref.rdp_mask(l, 2.0) == 0).sum()) for l in floats) < sum(len(l) for l in floats) // 10


def test_the_stroke3_wrapper():
    s = np.array([[5, 5, 0], [1, 1, 0], [1, 1, 0], [1, 1, 1], [10, 0, 0], [0, 10, 2], [-10, 0, 0], [0, -10, 0]], np.int16)
    got = ref.simplify_stroke3(s, 2.0)
    # the first stroke is a straight line: its ends stay; the second is a closed square whose pen-2 row ends nothing
    assert got.dtype == np.float32 and got.tolist() == [[5, 5, 0], [3, 3, 1], [10, 0, 0], [0, 10, 2], [-10, 0, 0], [0, -10, 0]]
    assert ref.stroke_ranges(s[:, 2]) == [(0, 4), (4, 8)]
    assert ref.stroke_ranges(np.array([1, 1, 0, 1])) == [(0, 1), (1, 2), (2, 4)]
    assert ref.simplify_stroke3(np.zeros((0, 3), np.int16), 2.0).shape == (0, 3)
    pool = ref.sketch_pool()
    assert len(pool) == 2 * ref.OFFSETS_SCAN_BLOCK + 5
    named = pool[:130]
    assert any(len(s) == 0 for s in named) and any((s[:, 2] == 2).any() for s in named if len(s))
    assert any(len(s) > 6 and (s[:, 2] == 0).all() for s in named)                       # no pen lift
    assert any(((s[1:, 2] == 1) & (s[:-1, 2] == 1)).any() for s in named if len(s))     # one-point strokes
    assert {ref.LDS_POINTS - 1, ref.LDS_POINTS, ref.LDS_POINTS + 1, 64, 65} <= {len(s) for s in named}
    assert max(len(s) for s in named) > ref.LDS_POINTS + 40
    out = ref.simplify_all(named, 2.0)
    assert 3 * sum(len(o) for o in out) < sum(len(s) for s in named)                     # and the sketches shrink
    for s, o in zip(named, out):
        assert np.array_equal(o[:, :2].sum(0), np.asarray(s, np.float64)[:, :2].sum(0).astype(np.float32))
        assert (o[:, 2] == 1).sum() == (s[:, 2] == 1).sum()


# ---------------------------------------------------------------- host helpers
def test_scale_to_255():
    lines = [np.array([(10, 20), (30, 20)]), np.array([(20, 70)]), np.zeros((0, 2))]
    got = simplify.scale_to_255(lines)
    assert [g.dtype for g in got] == [np.float32] * 3 and got[2].shape == (0, 2)
    f = 255.0 / 50.0                                                         # the larger extent is y: 20 .. 70
    assert got[0].tolist() == [[0.0, 0.0], [np.float32(20 * f), 0.0]] and got[1].tolist() == [[np.float32(10 * f), 255.0]]
    # a drawing of extent 0 is aligned and otherwise left alone
    got = simplify.scale_to_255([np.array([(7, 9)]), np.array([(7, 9), (7, 9)])])
    assert got[0].tolist() == [[0, 0]] and got[1].tolist() == [[0, 0], [0, 0]]
    assert simplify.scale_to_255([]) == []


def test_drawing_to_stroke3():
    drawing = [np.array([(1.4, 2.6), (4.5, 2.5), (10.0, 0.2)]), np.zeros((0, 2)), np.array([(3, 3)]), np.array([(0, 8), (0, 0)])]
    got = simplify.drawing_to_stroke3(drawing)
    # np.rint rounds halves to even: 4.5 -> 4, 2.5 -> 2; the single-point stroke is one row with pen 1
    assert got.dtype == np.int16
    assert got.tolist() == [[1, 3, 0], [3, -1, 0], [6, -2, 1], [-7, 3, 1], [-3, 5, 0], [0, -8, 1]]
    assert simplify.drawing_to_stroke3([]).shape == (0, 3) and simplify.drawing_to_stroke3([np.zeros((0, 2))]).shape == (0, 3)
    with pytest.raises(ValueError):
        simplify.drawing_to_stroke3([np.array([(0, 0), (40000, 0)])])
    raw = [[[1, 2, 3], [4, 5, 6], [0, 10, 20]], [[], [], []], [[7], [8]]]
    lines = simplify.quickdraw_lines(raw)
    assert [l.tolist() for l in lines] == [[[1, 4], [2, 5], [3, 6]], [[7, 8]]]
    with pytest.raises(ValueError):
        simplify.quickdraw_lines([[[1, 2], [3]]])


def test_integer_sketches_must_stay_where_fp32_is_exact():
    """Refused on the host, before anything touches a device: an integer sketch whose running position reaches 2^23, where the
    fp32 sums and the offsets between kept rows would stop being exact integers."""
    far = np.array([[1 << 22, 0, 0], [1 << 22, 0, 0], [1, 1, 1]], np.int32)
    near = np.array([[1, 1, 0], [2, 2, 1]], np.int32)
    with pytest.raises(ValueError, match="sketch 2"):
        simplify.simplify_sketches([near, np.zeros((0, 3), np.int16), far], 2.0)
    with pytest.raises(ValueError, match="sketch 0"):
        simplify.simplify_sketches([np.array([[0, -(1 << 25) - 1, 1]], np.int64)], 2.0)     # an offset the packing rounds


def test_the_scripts_ask_for_the_class_list():
    import runpy
    for script in ("prepare-distributed-quickdraw.py", os.path.join("quickdraw", "simplify_ndjson.py")):
        main = runpy.run_path(os.path.join(ROOT, "prep_data", script))["main"]
        with pytest.raises(SystemExit):
            main(["--dataset-dir", "a", "--ndjson-dir", "a", "--target-dir", "b"])


def test_the_device_functions_have_no_cpu_fallback():
    import torch
    from sketchformer_amd import _lib, ops
    with pytest.raises(_lib.SkfError):
        ops.rdp_keep(torch.zeros(4, 2), torch.tensor([0, 4]), 2.0)
    with pytest.raises(_lib.SkfError):
        ops.stroke3_simplify(torch.zeros(4, 3), torch.tensor([0, 4]), 2.0)


def test_workspace_queries():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    lib = _lib.load()
    for P, N in ((0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3)):
        assert lib.skf_stroke3_simplify_workspace_bytes(P, N) == 0, (P, N)
    for P in (0, -1, 1 << 31):
        assert lib.skf_rdp_workspace_bytes(P) == 0
    sizes = [lib.skf_stroke3_simplify_workspace_bytes(P, 7) for P in (1, 64, 1000, 100000, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 13 * ((1 << 31) - 1)
    assert lib.skf_rdp_workspace_bytes(1000) >= 5 * 1000
    header = open(os.path.join(ROOT, "include", "skf.h")).read()
    from sketchformer_amd import ops
    assert "#define SKF_RDP_LDS_POINTS %d\n" % ref.LDS_POINTS in header and ops.RDP_LDS_POINTS == ref.LDS_POINTS


# ---------------------------------------------------------------- the chunk script against the reference's files
def _same_npz(got_path, want_path):
    with np.load(got_path, allow_pickle=True) as got, np.load(want_path, allow_pickle=True) as want:
        assert sorted(got.files) == sorted(want.files)
        for key in want.files:
            g, w = got[key], want[key]
            assert g.dtype == w.dtype and g.shape == w.shape, (want_path, key, g.dtype, w.dtype)
            if w.dtype == object:
                assert all(p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q) for p, q in zip(g, w)), key
            else:
                assert g.tobytes() == w.tobytes(), (want_path, key, g, w)      # the statistics bit for bit


@pytest.mark.parametrize("cut", [0, 1])
def test_the_chunk_script_writes_what_the_reference_wrote(cut, tmp_path, capsys):
    target = tmp_path / "chunks"
    ref.run_chunk_script(target, "--cut-chunks", str(cut), "--simplify-epsilon", "0")
    want = os.path.join(GOLDEN, "cut%d" % cut)
    names = sorted(os.listdir(want))
    assert names == sorted(os.listdir(str(target))) and len(names) == 5 - cut
    for name in names:
        _same_npz(os.path.join(str(target), name), os.path.join(want, name))
    with np.load(os.path.join(want, "meta.npz")) as meta, np.load(os.path.join(want, "train_000.npz"), allow_pickle=True) as c0:
        if cut:                                                              # the quirk: one chunk's std, still divided by two
            assert meta["std"] == c0["std"] / 2 and meta["n_samples_train"] == 18
