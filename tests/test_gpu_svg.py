"""The SVG pipeline of sketchformer_amd/svg.py on the device against the host composition of the three rules it chains: the
flattening restatement (tests/flatten_reference.py), the reference's normalisation in numpy float64, and the RDP restatement
(tests/simplify_reference.py).  Equality on bit patterns throughout."""
import os
import runpy
import shutil

import numpy as np
import pytest

import flatten_reference as fr
import simplify_reference as ref
from sketchformer_amd import ops, simplify, svg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "svg")
NAMES = ("curves", "shapes", "grammar", "erased")
FILES = [os.path.join(GOLDEN, n + ".svg") for n in NAMES]


def _framed(drawing):
    """the working frame, restated: the box of the control points to the origin, its larger side to 1024, in float64"""
    every = np.concatenate([c.reshape(-1, 2) for c, _ in drawing])
    lo = every.min(axis=0)
    extent = (every.max(axis=0) - lo).max()
    return [((c - lo) * (1024.0 / extent), k) for c, k in drawing]


def _host_polylines(path, tol):
    return [fr.flatten_subpath(c, k, tol) for c, k in _framed(svg.parse_svg(path))]


def _host_stroke3(path, scale=100.0, epsilon=1.5, tol=0.0625, omit_first_point=True):
    """flatten_reference, the reference's normalisation as single float64 operations, simplify_reference's RDP, lines_to_strokes"""
    lines = _host_polylines(path, tol)
    every = np.concatenate(lines)
    assert every.dtype == np.float32
    lo, hi = every.min(axis=0).astype(np.float64), every.max(axis=0).astype(np.float64)
    max_hw = (hi - lo).max()
    rows = []
    for line in lines:
        norm = ((((line.astype(np.float64) - lo) / max_hw) * 2.0 - 1.0) * np.float64(scale)).astype(np.float32)
        kept = norm[ref.rdp_mask(norm, epsilon) != 0]
        pen = np.zeros((len(kept), 1))
        pen[-1] = 1
        rows.append(np.concatenate([kept.astype(np.float64), pen], axis=1))
    strokes = np.concatenate(rows)
    strokes[1:, 0:2] = strokes[1:, 0:2] - strokes[:-1, 0:2]
    return (strokes[1:] if omit_first_point else strokes).astype(np.float32)


@pytest.fixture(scope="module")
def host():
    return [_host_stroke3(f) for f in FILES]


def test_svg_to_stroke3_is_the_host_composition(host):
    got = svg.svg_to_stroke3(FILES)
    assert len(got) == 4
    for name, g, w in zip(NAMES, got, host):
        print("%s: %d rows of stroke-3, %d strokes" % (name, len(g), int(g[:, 2].sum())))
        assert g.dtype == np.float32 and g.shape == w.shape and g.shape[1] == 3 and len(g) >= 20, name
        assert fr.same_bits(g, w), name
    # one at a time, from text and from parsed drawings, with the first point kept, at another scale and tolerance
    alone = svg.svg_to_stroke3([open(FILES[0]).read()])[0]
    assert fr.same_bits(alone, host[0])
    other = svg.svg_to_stroke3([svg.parse_svg(FILES[1])], scale=255.0, epsilon=2.0, tol=0.5, omit_first_point=False)[0]
    assert fr.same_bits(other, _host_stroke3(FILES[1], scale=255.0, epsilon=2.0, tol=0.5, omit_first_point=False))
    assert other[0, :2].tolist() != [0.0, 0.0]


def test_read_svg_returns_the_layout_of_the_reference(host):
    for path, w in zip(FILES, host):
        s = svg.read_svg(path)
        assert fr.same_bits(s, w) and s.dtype == np.float32 and s.ndim == 2 and s.shape[1] == 3
        n_strokes = len(svg.parse_svg(path))
        assert set(np.unique(s[:, 2]).tolist()) == {0.0, 1.0} and int(s[:, 2].sum()) == n_strokes and s[-1, 2] == 1
        whole = svg.svg_to_stroke3([path], omit_first_point=False)[0]
        assert fr.same_bits(whole[1:], s)                                     # the first point is what is left out
        pos = np.cumsum(whole[:, :2].astype(np.float64), axis=0)
        assert np.abs(pos).max() <= 100.0 + 1e-3                              # inside +-scale ...
        span = (pos.max(axis=0) - pos.min(axis=0)).max()                      # ... the larger side spanning all of it, but for what
        assert 200.0 - 2 * 1.5 <= span <= 200.0 + 1e-3                        # RDP may drop: an extreme point within epsilon, each side
    half = svg.read_svg(FILES[0], scale=50.0, draw_mode=True)
    assert fr.same_bits(half, _host_stroke3(FILES[0], scale=50.0))


def test_drawings_without_ink_and_of_no_extent():
    blank = "<svg><text>nothing</text><path d='M5 5'/></svg>"
    dot = "<svg><path d='M7 7 L7 7'/></svg>"
    got = svg.svg_to_stroke3([blank, FILES[3], dot, blank], omit_first_point=False)
    assert got[0].shape == (0, 3) and got[3].shape == (0, 3) and got[0].dtype == np.float32
    assert fr.same_bits(got[1], _host_stroke3(FILES[3], omit_first_point=False))
    assert got[2].tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]              # aligned, not scaled
    assert [g.shape for g in svg.svg_to_stroke3([blank, dot])] == [(0, 3), (1, 3)]
    assert svg.svg_to_stroke3([]) == [] and svg.flatten_paths([[], []], 0.25) == [[], []]


def test_a_small_row_budget_gives_the_same_batch(host, monkeypatch):
    sources = FILES + ["<svg/>"] + FILES[::-1]
    calls = []
    real = ops.path_flatten
    monkeypatch.setattr(ops, "path_flatten", lambda *a: calls.append(int(a[2].shape[0]) - 1) or real(*a))
    whole = svg.svg_to_stroke3(sources)
    assert len(calls) == 1
    del calls[:]
    cut = svg.svg_to_stroke3(sources, row_budget=400)
    assert len(calls) >= 4 and sum(calls) == 2 * sum(len(svg.parse_svg(f)) for f in FILES)
    for w, c, h in zip(whole, cut, host + [np.zeros((0, 3), np.float32)] + host[::-1]):
        assert fr.same_bits(w, h) and fr.same_bits(c, h)
    with pytest.raises(ValueError, match="budget"):
        svg.svg_to_stroke3(sources, row_budget=0)


def test_flatten_paths_is_the_restatement():
    drawings = [svg.parse_svg(f) for f in FILES]
    got = svg.flatten_paths(drawings + [[]], 0.25, row_budget=300)
    assert got[4] == []
    for d, g in zip(drawings, got):
        assert len(g) == len(d)
        for (c, k), line in zip(d, g):
            assert line.dtype == np.float32 and fr.same_bits(line, fr.flatten_subpath(c, k, 0.25))


def test_convert_svg_dataset_script(tmp_path, capsys):
    """12 usable files a class -> 10 train, 1 valid, 1 test, in sorted name order; a broken file and one without ink are reported
    and skipped; the chunk script takes the result as it takes the QuickDraw class files."""
    root, out, chunks = tmp_path / "svg", tmp_path / "classes", tmp_path / "chunks"
    order = {}
    for cls, shift in (("cat", 0), ("dog", 1)):
        (root / cls).mkdir(parents=True)
        order[cls] = []
        for i in range(12):
            src = FILES[(i + shift) % 4]
            shutil.copy(src, str(root / cls / ("%02d.svg" % i)))
            order[cls].append(src)
    (root / "cat" / "03b_broken.svg").write_text("<svg><path d='M0 0 L5'/></svg>")
    (root / "dog" / "zz_blank.svg").write_text("<svg/>")
    (root / "dog" / "notes.txt").write_text("not a drawing")
    (tmp_path / "list.txt").write_text("cat\ndog\n")
    script = os.path.join(ROOT, "prep_data", "svg", "convert_svg_dataset.py")
    skipped = runpy.run_path(script)["main"](["--svg-dir", str(root), "--class-list", str(tmp_path / "list.txt"), "--target-dir", str(out)])
    printed = capsys.readouterr().out
    assert skipped == 2 and "2 files skipped" in printed
    assert str(root / "cat" / "03b_broken.svg") in printed and "position 7" in printed and str(root / "dog" / "zz_blank.svg") in printed

    def want(path):
        lines = simplify.scale_to_255(_host_polylines(path, 0.0625))
        return simplify.drawing_to_stroke3([l[ref.rdp_mask(l, 2.0) != 0] for l in lines])

    wanted = {f: want(f) for f in FILES}
    for cls in ("cat", "dog"):
        with np.load(str(out / (cls + ".npz")), allow_pickle=True) as npz:
            assert sorted(npz.files) == ["test", "train", "valid"]
            parts = [npz["train"], npz["valid"], npz["test"]]
        assert [len(p) for p in parts] == [10, 1, 1]
        for got, src in zip(np.concatenate(parts), order[cls]):
            assert got.dtype == np.int16 and got.shape[1] == 3 and np.array_equal(got, wanted[src]), (cls, src)
            assert got[:, :2].cumsum(axis=0).max() <= 255 and got[:, :2].cumsum(axis=0).min() >= 0
    main = runpy.run_path(os.path.join(ROOT, "prep_data", "prepare-distributed-quickdraw.py"))["main"]
    main(["--dataset-dir", str(out), "--class-list", str(tmp_path / "list.txt"), "--n-chunks", "2", "--n-classes", "2", "--target-dir", str(chunks)])
    with np.load(str(chunks / "train_000.npz"), allow_pickle=True) as npz:
        assert len(npz["x"]) == 10 and npz["y"].tolist() == [0] * 5 + [1] * 5 and npz["label_names"].tolist() == ["cat", "dog"]
        assert np.array_equal(npz["x"][0], wanted[FILES[0]]) and np.array_equal(npz["x"][5], wanted[FILES[1]])
    with np.load(str(chunks / "meta.npz"), allow_pickle=True) as npz:
        assert int(npz["n_samples_train"]) == 20 and int(npz["n_samples_valid"]) == 2 and int(npz["n_samples_test"]) == 2
    for bad in (["--tol", "0"], ["--tol", "nan"], ["--resample-spacing", "-1"], ["--valid-fraction", "0.7", "--test-fraction", "0.6"]):
        with pytest.raises(SystemExit):
            runpy.run_path(script)["main"](["--svg-dir", "a", "--class-list", "b", "--target-dir", "c"] + bad)
