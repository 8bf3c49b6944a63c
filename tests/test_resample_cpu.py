"""Arc-length resampling, the parts that need no GPU: the facts of the host restatement (tests/resample_reference.py) that give
tests/test_gpu_resample.py its teeth, the host-side refusals of sketchformer_amd.simplify, and the option of the QuickDraw script
with the device call replaced by the restatement."""
import json
import os
import runpy

import numpy as np
import pytest

import resample_reference as rr
import simplify_reference as ref
from sketchformer_amd import simplify

ROOT = ref.ROOT


def _pools():
    return [l for l in ref.int_pool() + ref.float_pool()]


# ---------------------------------------------------------------- the restatement
def test_the_count_formula():
    for total, step, want in ((0, 65536, 1), (1, 65536, 2), (65536, 65536, 2), (65537, 65536, 3), (10 * 65536, 65536, 11),
                              (10 * 65536, 3 * 65536, 5), (5, 7, 2)):
        assert rr.n_rows(total, step) == want, (total, step)
    for line in _pools():
        for spacing in (1.0, 2.5, 1e6):
            q, C = rr.arc_table(line) if len(line) else (None, np.zeros(1, np.int64))
            out = rr.resample(line, spacing)
            assert out.dtype == np.float32
            assert len(out) == (0 if len(line) == 0 else rr.n_rows(C[-1], rr.step_of(spacing))), (len(line), spacing)
    assert rr.step_of(1.0) == 65536 and rr.step_of(2.5) == 163840 and rr.step_of(2.0 ** -16) == 1
    for bad in (0.0, -1.0, 2.0 ** -17, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rr.step_of(bad)


def test_the_ends_are_copied_bit_for_bit():
    for line in _pools():
        if len(line) == 0:
            continue
        for out in (rr.resample(line, 1.0), rr.resample(line, 2.5), rr.resample_n(line, 33)):
            assert rr.same_bits(out[-1], line[-1])
            if len(out) > 1:
                assert rr.same_bits(out[0], line[0])
    far = rr.resample(rr.LINE_0_10, 1e6)                                        # a spacing above the length: the two ends
    assert rr.same_bits(far, rr.LINE_0_10)


def test_the_integer_grid_fixtures_are_exact():
    out = rr.resample(rr.LINE_0_10, 1.0)
    assert out.tolist() == [[float(k), 0.0] for k in range(11)]
    q, C = rr.arc_table(rr.PYTHAGORAS)
    assert q.tolist() == [5 * 65536] * 4 and C.tolist() == [0, 327680, 655360, 983040, 1310720]
    out = rr.resample(rr.PYTHAGORAS, 1.0)
    assert len(out) == 21
    p = rr.PYTHAGORAS.astype(np.float64)
    for k in range(21):
        i, j = min(k // 5, 3), k - 5 * min(k // 5, 3)
        want = (p[i] + (j / 5.0) * (p[i + 1] - p[i])).astype(np.float32)         # exact fifths along every segment
        assert rr.same_bits(out[k], want), k
    assert rr.same_bits(out[::5], rr.PYTHAGORAS)                                # the vertices themselves
    assert out[1].tolist() == [np.float32(0.6), np.float32(0.8)]


def test_zero_length_and_single_point_polylines():
    one = np.array([[3.5, -2.25]], np.float32)
    same = np.repeat(one, 5, axis=0)
    for line in (one, same):
        assert rr.same_bits(rr.resample(line, 1.0), one)
        assert rr.same_bits(rr.resample_n(line, 4), np.repeat(one, 4, axis=0))
    assert rr.resample(np.zeros((0, 2)), 1.0).shape == (0, 2)
    assert rr.same_bits(rr.resample_n(np.zeros((0, 2)), 3), np.zeros((3, 2), np.float32))
    # a zero-length segment inside a polyline is never chosen: the duplicate changes nothing
    dup = np.array([(0, 0), (3, 4), (3, 4), (3, 4), (6, 0)], np.float32)
    assert rr.same_bits(rr.resample(dup, 1.0), rr.resample(dup[[0, 1, 4]], 1.0))


def test_a_polyline_does_not_depend_on_its_neighbours():
    lines = rr.random_int_strokes(12)
    alone = [rr.resample(l, 1.0) for l in lines]
    xy, offsets = rr.pack(rr.resample_all(lines[::-1], 1.0))
    for i, l in enumerate(lines[::-1]):
        assert rr.same_bits(xy[offsets[i]:offsets[i + 1]], alone[len(lines) - 1 - i])


def test_consecutive_outputs_are_at_most_a_spacing_apart():
    grown = [0, 0]
    for line in rr.random_int_strokes(2000) + [l for l in _pools() if len(l)]:
        for spacing in (1.0, 2.5):
            out = rr.resample(line, spacing).astype(np.float64)
            gaps = np.hypot(*(out[1:] - out[:-1]).T)
            assert gaps.size == 0 or gaps.max() <= spacing + 1e-3
        grown[0] += len(line)
        grown[1] += len(rr.resample(line, 1.0))
    assert grown[1] > 5 * grown[0]                                              # resampling at one pixel grows the data


@pytest.mark.parametrize("n_out", [2, 33, 64, 65, 256])
def test_count_mode_rows_ends_and_targets(n_out):
    for line in _pools():
        out = rr.resample_n(line, n_out)
        assert out.shape == (n_out, 2) and out.dtype == np.float32
        if len(line):
            assert rr.same_bits(out[0], line[0]) or rr.arc_table(line)[1][-1] == 0
            assert rr.same_bits(out[-1], line[-1]) or rr.arc_table(line)[1][-1] == 0
    for total in (0, 1, 5, n_out - 2, n_out - 1, n_out, 65536 * 255, (1 << 62) + 12345, (1 << 63) - 1):
        assert rr.count_targets(total, n_out).tolist() == rr.count_targets_exact(total, n_out), total


def test_count_mode_on_the_fixture():
    out = rr.resample_n(rr.PYTHAGORAS, 5)
    assert rr.same_bits(out, rr.PYTHAGORAS)
    out = rr.resample_n(rr.LINE_0_10, 11)
    assert out.tolist() == [[float(k), 0.0] for k in range(11)]
    with pytest.raises(ValueError):
        rr.resample_n(rr.LINE_0_10, 1)
    with pytest.raises(ValueError):
        rr.resample_n(rr.LINE_0_10, rr.MAX_N + 1)


# ---------------------------------------------------------------- host-side checks, no device involved
def test_resample_lines_refuses_bad_arguments_on_the_host():
    line = [np.array([(0, 0), (10, 0)], np.float64)]
    with pytest.raises(ValueError, match="exactly one"):
        simplify.resample_lines(line)
    with pytest.raises(ValueError, match="exactly one"):
        simplify.resample_lines(line, spacing=1.0, n_points=4)
    for bad in (0.0, -1.0, 2.0 ** -17, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="spacing"):
            simplify.resample_lines(line, spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            simplify.simplify_lines(line, 2.0, resample_spacing=bad)
    for bad in (1, 0, -3, 65537):
        with pytest.raises(ValueError, match="n_points"):
            simplify.resample_lines(line, n_points=bad)
    assert simplify.RESAMPLE_MAX_COORD == rr.MAX_COORD
    for bad in (rr.MAX_COORD + 1.0, -rr.MAX_COORD - 1.0, float("nan"), float("inf")):
        far = [line[0], np.array([(0, 0), (bad, 0)], np.float64)]
        with pytest.raises(ValueError, match="16384"):
            simplify.resample_lines(far, spacing=1.0)
        with pytest.raises(ValueError, match="16384"):
            simplify.resample_lines(far, n_points=8)
        with pytest.raises(ValueError, match="16384"):
            simplify.simplify_lines(far, 2.0, resample_spacing=1.0)
    # nothing to resample: answered on the host
    empty = simplify.resample_lines([np.zeros((0, 2)), np.zeros((0, 2))], spacing=1.0)
    assert [e.shape for e in empty] == [(0, 2), (0, 2)]
    empty = simplify.resample_lines([np.zeros((0, 2))], n_points=3)
    assert empty[0].shape == (3, 2) and not empty[0].any()
    assert [e.shape for e in simplify.simplify_lines([np.zeros((0, 2))], 2.0, resample_spacing=1.0)] == [(0, 2)]


def test_the_row_budget_cuts():
    offsets = np.array([0, 5, 5, 9, 30, 31, 40], np.int64)
    assert simplify._cut_by_rows(offsets, 10) == [(0, 3), (3, 4), (4, 6)]       # a polyline above the budget goes alone
    assert simplify._cut_by_rows(offsets, 1000) == [(0, 6)]
    assert simplify._cut_by_rows(offsets, 1) == [(i, i + 1) for i in range(6)]
    with pytest.raises(ValueError):
        simplify._cut_by_rows(offsets, 0)


def test_the_device_functions_have_no_cpu_fallback():
    import torch
    from sketchformer_amd import _lib, ops
    with pytest.raises(_lib.SkfError):
        ops.polyline_resample(torch.zeros(4, 2), torch.tensor([0, 4]), 1.0)
    with pytest.raises(_lib.SkfError):
        ops.polyline_resample_n(torch.zeros(4, 2), torch.tensor([0, 4]), 8)


def test_workspace_query_and_header_constants():
    from sketchformer_amd import build, _lib, ops
    build.build_library(verbose=False)
    lib = _lib.load()
    for P, S in ((0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3)):
        assert lib.skf_polyline_resample_workspace_bytes(P, S) == 0, (P, S)
    assert lib.skf_polyline_resample_workspace_bytes(1000, 7) >= 8 * 1000 + 4 * 7
    header = open(os.path.join(ROOT, "include", "skf.h")).read()
    assert "#define SKF_RESAMPLE_MAX_N %d\n" % rr.MAX_N in header and ops.RESAMPLE_MAX_N == rr.MAX_N
    assert "#define SKF_RESAMPLE_MAX_COORD %d\n" % rr.MAX_COORD in header and ops.RESAMPLE_MAX_COORD == rr.MAX_COORD
    assert "skf_resample.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCE_FLAGS["skf_resample.hip"]
    assert "#pragma clang fp contract(off)" in open(os.path.join(build.CSRC, "skf_resample.hip")).read()


# ---------------------------------------------------------------- the QuickDraw script, the device call replaced
def _host_simplify_lines(lines, epsilon, device=None, resample_spacing=None):
    lines = [np.asarray(l).reshape(-1, 2) for l in lines]
    if resample_spacing is not None:
        lines = rr.resample_all(lines, resample_spacing)
    return [l[ref.rdp_mask(l, epsilon) != 0] for l in lines]


def _records():
    rng = np.random.RandomState(37)
    records = []
    for _ in range(5):
        drawing = []
        for _ in range(int(rng.randint(1, 4))):
            n = int(rng.randint(2, 40))
            p = ref.smooth_int_stroke(rng, n) * 3 + 100
            drawing.append([p[:, 0].tolist(), p[:, 1].tolist()])
        records.append({"word": "thing", "recognized": True, "drawing": drawing})
    return records


def _run_script(tmp_path, name, *extra):
    raw, out = tmp_path / "raw", tmp_path / name
    raw.mkdir(exist_ok=True)
    with open(str(raw / "thing.ndjson"), "w") as f:
        f.write("\n".join(json.dumps(r) for r in _records()) + "\n")
    with open(str(tmp_path / "list.txt"), "w") as f:
        f.write("thing\n")
    main = runpy.run_path(os.path.join(ROOT, "prep_data", "quickdraw", "simplify_ndjson.py"))["main"]
    main(["--ndjson-dir", str(raw), "--class-list", str(tmp_path / "list.txt"), "--target-dir", str(out), "--n-train", "3",
          "--n-valid", "1", "--n-test", "1"] + list(extra))
    with np.load(str(out / "thing.npz"), allow_pickle=True) as npz:
        return list(npz["train"]) + list(npz["valid"]) + list(npz["test"])


def test_the_script_option(tmp_path, monkeypatch):
    calls = []

    def spy(lines, epsilon, device=None, **kw):
        calls.append(dict(kw))
        return _host_simplify_lines(lines, epsilon, device, **kw)

    monkeypatch.setattr(simplify, "simplify_lines", spy)
    today = []
    for r in _records():
        lines = simplify.scale_to_255(simplify.quickdraw_lines(r["drawing"]))
        today.append(simplify.drawing_to_stroke3([l[ref.rdp_mask(l, 2.0) != 0] for l in lines]))
    off = _run_script(tmp_path, "off")
    assert calls == [{}]                                                        # the default is today's call, keyword and all
    zero = _run_script(tmp_path, "zero", "--resample-spacing", "0")
    assert calls == [{}, {}]
    for got in (off, zero):
        assert len(got) == len(today)
        for g, w in zip(got, today):
            assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w)
    on = _run_script(tmp_path, "on", "--resample-spacing", "1.0")
    assert calls[2] == {"resample_spacing": 1.0}
    want = []
    for r in _records():
        lines = rr.resample_all(simplify.scale_to_255(simplify.quickdraw_lines(r["drawing"])), 1.0)
        want.append(simplify.drawing_to_stroke3([l[ref.rdp_mask(l, 2.0) != 0] for l in lines]))
    for g, w in zip(on, want):
        assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w)
    assert any(g.shape != w.shape or not np.array_equal(g, w) for g, w in zip(on, today))      # on changes the files
    for g, r in zip(on, _records()):
        assert int((g[:, 2] == 1).sum()) == len(r["drawing"])                   # stroke ends stay
    main = runpy.run_path(os.path.join(ROOT, "prep_data", "quickdraw", "simplify_ndjson.py"))["main"]
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            main(["--ndjson-dir", "a", "--class-list", "b", "--target-dir", "c", "--resample-spacing", bad])


# ---------------------------------------------------------------- the alignment side: defaults stay off
def test_the_dtw_keyword_and_the_experiment_hparam_default_to_off():
    import inspect
    from sketchformer_amd import align, experiments
    assert inspect.signature(align.sketch_dtw).parameters["resample"].default is None
    assert inspect.signature(simplify.simplify_lines).parameters["resample_spacing"].default is None
    Exp = experiments.get_experiment_by_name("sequence-retrieval")
    assert dict(Exp.default_hparams().values())["resample_points"] == 0
    h = dict(Exp.parse_hparams("distance=dtw,resample_points=64").values())
    assert (h["distance"], h["resample_points"]) == ("dtw", 64)
