"""Device stroke simplification against the host restatement of tests/simplify_reference.py (tests/test_simplify_cpu.py asserts
the fixtures' teeth on the CPU).  Everything is equality - masks, rows as bit patterns, offsets, dtypes and shapes - there are no
tolerances."""
import json
import os
import runpy

import numpy as np
import pytest
import torch

import simplify_reference as ref
from sketchformer_amd import _lib, ops, preprocess, simplify

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT, GOLDEN = ref.ROOT, ref.GOLDEN
ABOVE_THE_SCAN_BLOCK = 2 * ref.OFFSETS_SCAN_BLOCK + 5
EPSILONS = (0.0, 1.0, 2.0, 4.5, 1e9)
STROKE_COUNTS = (1, 63, 64, 65, ABOVE_THE_SCAN_BLOCK)
SKETCH_COUNTS = (1, 63, 64, 65, 130, ABOVE_THE_SCAN_BLOCK)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # (a copy: the shared references are read-only)


def _keep(lines, epsilon):
    xy, offsets = ref.pack_lines(lines)
    keep = ops.rdp_keep(_dev(xy), _dev(offsets), epsilon)
    assert keep.dtype == torch.uint8 and tuple(keep.shape) == (len(xy),)
    return keep.cpu().numpy()


def test_the_header_constant_is_the_one_the_pools_straddle():
    assert ops.RDP_LDS_POINTS == ref.LDS_POINTS
    assert {ref.LDS_POINTS - 1, ref.LDS_POINTS, ref.LDS_POINTS + 1, ref.LDS_POINTS + 5, 0, 1, 2, 3, 4, 63, 64, 65, 130} == set(ref.STROKE_LENGTHS)


# ---------------------------------------------------------------- ops.rdp_keep
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("kind", ["integer", "float"])
def test_rdp_keep_matches_the_restatement(kind, epsilon):
    lines = ref.int_pool() if kind == "integer" else ref.float_pool()
    got, want = _keep(lines, epsilon), ref.masks(lines, epsilon)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    if kind == "integer" and epsilon == 2.0:
        assert 2 * int((want == 0).sum()) > len(want) - 2 * len(lines)     # and most of the interior went


def test_rdp_keep_on_the_named_fixtures():
    named = [ref.TENT, ref.SQUARE, ref.COLLINEAR] + [(ref.zigzag(n), 2.0, [1] * n) for n in ref.ZIGZAG_LENGTHS + (ref.LDS_POINTS + 5,)]
    for points, epsilon, want in named:
        assert ref.rdp_mask(points, epsilon).tolist() == want
        assert _keep([points], epsilon).tolist() == want, (len(points), epsilon)
    # all of them in one call, next to each other, at one epsilon
    lines = [p for p, _, _ in named]
    assert np.array_equal(_keep(lines, 2.0), ref.masks(lines, 2.0))
    # a zigzag flattened by a large epsilon keeps its ends, on chip and from the workspace
    for n in (257, ref.LDS_POINTS + 5):
        assert _keep([ref.zigzag(n)], 1e9).tolist() == [1] + [0] * (n - 2) + [1]


@pytest.mark.parametrize("S", STROKE_COUNTS)
def test_rdp_keep_stroke_counts(S):
    lines = ref.short_strokes(ABOVE_THE_SCAN_BLOCK)[:S]
    if sum(len(l) for l in lines) == 0:
        lines = lines + [ref.TENT[0]]
    assert np.array_equal(_keep(lines, 1.0), ref.masks(lines, 1.0))


def test_rdp_keep_reads_rows_of_any_stride_and_leaves_its_inputs_alone():
    lines = ref.int_pool()[:12]
    xy, offsets = ref.pack_lines(lines)
    wide = torch.full((len(xy), 5), float("nan"), device=DEV)
    wide[:, 1:3] = _dev(xy)
    off_d = _dev(offsets)
    view = wide[:, 1:3]
    first = ops.rdp_keep(view, off_d, 2.0)
    again = ops.rdp_keep(view, off_d, 2.0)
    assert torch.equal(first, again) and np.array_equal(first.cpu().numpy(), ref.masks(lines, 2.0))
    assert np.array_equal(view.cpu().numpy(), xy) and np.array_equal(off_d.cpu().numpy(), offsets)


# ---------------------------------------------------------------- ops.stroke3_simplify
@pytest.fixture(scope="module")
def pool():
    pool = ref.sketch_pool()
    assert len(pool) == max(SKETCH_COUNTS)
    return pool


_WANT = {}


def _want(pool, epsilon):
    """The restatement of the whole pool, once per epsilon; a prefix of the pool gives a prefix of it."""
    if epsilon not in _WANT:
        _WANT[epsilon] = ref.simplify_all(pool, epsilon)
    return _WANT[epsilon]


def _simplify(sketches, epsilon):
    flat, offsets = preprocess.pack_ragged(sketches)
    return ops.stroke3_simplify(_dev(flat), _dev(offsets), epsilon)


def _assert_is(got, want):
    out_flat, out_offsets = got
    flat, offsets = preprocess.pack_ragged(want)
    assert out_flat.dtype == torch.float32 and out_offsets.dtype == torch.int64
    assert tuple(out_offsets.shape) == offsets.shape and tuple(out_flat.shape) == flat.shape and out_flat.is_contiguous()
    assert np.array_equal(out_offsets.cpu().numpy(), offsets)
    bits, want_bits = out_flat.cpu().numpy().view(np.int32), flat.view(np.int32)
    assert np.array_equal(bits, want_bits), np.argwhere(bits != want_bits)[:5]


@pytest.mark.parametrize("N", SKETCH_COUNTS)
@pytest.mark.parametrize("epsilon", [1.0, 2.0])
def test_stroke3_simplify_matches_the_restatement(epsilon, N, pool):
    _assert_is(_simplify(pool[:N], epsilon), _want(pool, epsilon)[:N])


@pytest.mark.parametrize("epsilon", [0.0, 4.5, 1e9])
def test_stroke3_simplify_at_the_other_epsilons(epsilon, pool):
    named = pool[:130]
    want = ref.simplify_all(named, epsilon)
    _assert_is(_simplify(named, epsilon), want)
    if epsilon == 1e9:                                                       # nothing but stroke ends and stroke starts is left
        for s, w in zip(named, want):
            ends = set(np.flatnonzero(np.asarray(s)[:, 2] == 1).tolist())
            seeds = ({0, len(s) - 1} | ends | {e + 1 for e in ends}) & set(range(len(s)))
            assert len(w) == len(seeds)


def test_stroke3_simplify_on_float_offsets():
    """Offsets that are no integers: the fp32 running sum rounds, and the rows are still the restatement's bit for bit."""
    rng = np.random.RandomState(35)
    sketches = []
    for n in (1, 2, 7, 64, 65, 200, ref.LDS_POINTS + 9):
        s = np.zeros((n, 3), np.float32)
        s[:, :2] = rng.normal(0, 3, size=(n, 2)).astype(np.float32).cumsum(0) * 0.1 + rng.normal(0, 0.5, size=(n, 2))
        s[rng.randint(0, n, size=max(n // 40, 1)), 2] = 1
        sketches.append(s)
    for epsilon in (0.5, 2.0):
        want = ref.simplify_all(sketches, epsilon)
        _assert_is(_simplify(sketches, epsilon), want)
    assert sum(len(w) for w in want) < sum(len(s) for s in sketches)


def test_a_batch_is_the_concatenation_of_its_sketches_taken_alone(pool):
    named = pool[:14]
    out_flat, out_offsets = _simplify(named, 2.0)
    rows, offs = out_flat.cpu().numpy(), out_offsets.tolist()
    for i, s in enumerate(named):
        if len(s) == 0:
            assert offs[i] == offs[i + 1]
            continue
        alone_flat, alone_offsets = _simplify([s], 2.0)
        assert alone_offsets.tolist() == [0, offs[i + 1] - offs[i]]
        assert np.array_equal(alone_flat.cpu().numpy().view(np.int32), rows[offs[i]:offs[i + 1]].view(np.int32)), i


def test_two_calls_agree_bit_for_bit(pool):
    flat, offsets = preprocess.pack_ragged(pool)
    flat_d, off_d = _dev(flat), _dev(offsets)
    first = ops.stroke3_simplify(flat_d, off_d, 2.0)
    again = ops.stroke3_simplify(flat_d, off_d, 2.0)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    assert np.array_equal(flat_d.cpu().numpy(), flat) and np.array_equal(off_d.cpu().numpy(), offsets)   # the inputs are inputs


def test_a_sketch_keeps_its_extent_and_its_strokes(pool):
    out_flat, out_offsets = _simplify(pool, 2.0)
    rows, offs = out_flat.cpu().numpy(), out_offsets.tolist()
    assert offs[-1] == len(rows) < sum(len(s) for s in pool)
    for i, s in enumerate(pool):
        part = rows[offs[i]:offs[i + 1]]
        assert np.array_equal(part[:, :2].astype(np.int64).sum(0), np.asarray(s, np.int64)[:, :2].sum(0).reshape(2)), i
        assert int((part[:, 2] == 1).sum()) == int((np.asarray(s)[:, 2] == 1).sum()), i


def test_refusals():
    """SKF_EINVAL before anything is launched: the outputs keep what they held."""
    lib = _lib.load()
    flat = _dev(np.array([[1, 2, 0], [3, 4, 0], [2, -5, 1], [3, 3, 0], [2, 1, 1]], np.float32))
    offsets = _dev(np.array([0, 3, 5], np.int64))
    out_flat = torch.zeros(6, 3, dtype=torch.float32, device=DEV)
    out_offsets = torch.zeros(4, dtype=torch.int64, device=DEV)
    keep = torch.full((8,), 7, dtype=torch.uint8, device=DEV)
    ws_bytes = lib.skf_stroke3_simplify_workspace_bytes(5, 2)
    assert ws_bytes >= lib.skf_rdp_workspace_bytes(5) > 0
    ws = torch.zeros(ws_bytes + 64, dtype=torch.uint8, device=DEV)
    base = {"flat": flat.data_ptr(), "offsets": offsets.data_ptr(), "out_flat": out_flat.data_ptr(),
            "out_offsets": out_offsets.data_ptr(), "ws": ws.data_ptr(), "keep": keep.data_ptr()}

    def simp(P=5, N=2, epsilon=2.0, flags=0, ws_bytes=ws_bytes, shift=None):
        ptr = dict(base)
        if shift:
            ptr[shift[0]] += shift[1]
        return lib.skf_stroke3_simplify(ptr["flat"], P, ptr["offsets"], N, epsilon, flags, ptr["out_flat"], ptr["out_offsets"],
                                        ptr["ws"], ws_bytes, None)

    def rdp(P=5, S=2, ldp=3, epsilon=2.0, ws_bytes=ws_bytes, shift=None):
        ptr = dict(base)
        if shift:
            ptr[shift[0]] += shift[1]
        return lib.skf_rdp_f32(ptr["flat"], ldp, P, ptr["offsets"], S, epsilon, ptr["keep"], ptr["ws"], ws_bytes, None)

    for bad in (dict(N=0), dict(N=-1), dict(P=0), dict(P=1 << 31), dict(epsilon=-1e-9), dict(epsilon=float("nan")),
                dict(epsilon=float("inf")), dict(flags=1), dict(flags=2), dict(ws_bytes=8), dict(ws_bytes=ws_bytes - 1),
                dict(shift=("flat", 2)), dict(shift=("offsets", 4)), dict(shift=("out_flat", 1)), dict(shift=("out_offsets", 4)),
                dict(shift=("ws", 8))):
        assert simp(**bad) == -1, bad
    for bad in (dict(S=0), dict(S=-1), dict(P=0), dict(P=1 << 31), dict(ldp=1), dict(epsilon=-2.0), dict(epsilon=float("nan")),
                dict(epsilon=float("inf")), dict(ws_bytes=8), dict(shift=("flat", 2)), dict(shift=("offsets", 4)), dict(shift=("ws", 8))):
        assert rdp(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (out_flat == 0).all() and (out_offsets == 0).all() and (keep == 7).all()        # nothing was launched
    assert simp() == 0 and simp(epsilon=0.0) == 0 and rdp() == 0
    torch.cuda.synchronize()
    assert out_offsets.tolist()[:3] == [0, 3, 5] and keep.tolist() == [1, 1, 1, 1, 1, 7, 7, 7]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.stroke3_simplify(flat, offsets, bad)
        with pytest.raises(ValueError):
            ops.rdp_keep(flat[:, :2], offsets, bad)


# ---------------------------------------------------------------- end to end
def test_simplify_sketches_preserves_the_dtype_and_the_container(pool):
    named = pool[:40]
    want = _want(pool, 2.0)[:40]
    got = simplify.simplify_sketches(named, 2.0)
    assert isinstance(got, list) and len(got) == 40
    for g, w in zip(got, want):
        assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w)
    arr = np.empty(3, dtype=object)
    arr[0], arr[1], arr[2] = named[0].astype(np.int32), named[1].astype(np.float64), named[5]
    got = simplify.simplify_sketches(arr, 2.0)
    assert isinstance(got, np.ndarray) and got.dtype == object and got.shape == (3,)
    assert [g.dtype for g in got] == [np.int32, np.float32, np.int16] and got[2].shape == (0, 3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    empty = simplify.simplify_sketches([np.zeros((0, 3), np.int16)], 2.0)
    assert len(empty) == 1 and empty[0].shape == (0, 3)


def test_simplify_sketches_refuses_an_offset_its_dtype_cannot_hold():
    """The offset between kept rows is the sum of the dropped rows' offsets: 30000 + 10000 leaves int16 although both fit."""
    line = np.array([[0, 0, 0], [30000, 0, 0], [10000, 0, 1]], np.int16)
    with pytest.raises(ValueError, match="sketch 1.*int16"):
        simplify.simplify_sketches([line[:2], line], 2.0)
    got = simplify.simplify_sketches([line.astype(np.int32)], 2.0)[0]
    assert got.dtype == np.int32 and got.tolist() == [[0, 0, 0], [40000, 0, 1]]


def test_rdp_keep_takes_row_strides_and_refuses_overlapping_rows():
    lines = ref.int_pool()[:12]
    xy, offsets = ref.pack_lines(lines)
    wide = torch.zeros(len(xy), 5, device=DEV)
    wide[:, 1:3] = _dev(xy)
    got = ops.rdp_keep(wide[:, 1:3], _dev(offsets), 2.0)                     # a view into wider rows: ldp = 5
    assert np.array_equal(got.cpu().numpy(), ref.masks(lines, 2.0))
    one = torch.tensor([[3.0, 4.0]], device=DEV)
    two = torch.tensor([0, 2], device=DEV)
    for bad in (one.expand(2, 2), torch.arange(3.0, device=DEV).as_strided((2, 2), (1, 1))):      # row strides 0 and 1
        with pytest.raises(ValueError, match="overlap"):
            ops.rdp_keep(bad, two, 2.0)
    assert ops.rdp_keep(one.expand(1, 2), torch.tensor([0, 1], device=DEV), 2.0).tolist() == [1]   # a single row has no stride


def test_simplify_lines_returns_the_kept_points():
    lines = ref.int_pool()[:20]
    got = simplify.simplify_lines([l.astype(np.float64) for l in lines], 2.0)
    for g, l in zip(got, lines):
        assert g.dtype == np.float64 and np.array_equal(g, l[ref.rdp_mask(l, 2.0) != 0])


def _synthetic_records():
    rng = np.random.RandomState(36)
    records = []
    for r in range(6):
        drawing = []
        for _ in range(int(rng.randint(1, 5))):
            n = int(rng.randint(1, 60))
            p = ref.smooth_int_stroke(rng, n) * 3 + 100                      # raw drawings live on a larger canvas
            drawing.append([p[:, 0].tolist(), p[:, 1].tolist(), list(range(n))])
        records.append({"word": "thing", "recognized": r != 2, "drawing": drawing})
    records.append({"word": "thing", "recognized": True, "drawing": [[[5, 5], [9, 9], [0, 1]]]})      # extent 0
    return records


def test_simplify_ndjson_script(tmp_path):
    records = _synthetic_records()
    raw, out = tmp_path / "raw", tmp_path / "classes"
    raw.mkdir()
    with open(str(raw / "thing.ndjson"), "w") as f:
        f.write("\n".join(json.dumps(r) for r in records) + "\n")
    with open(str(tmp_path / "list.txt"), "w") as f:
        f.write("thing\n")
    script = os.path.join(ROOT, "prep_data", "quickdraw", "simplify_ndjson.py")
    runpy.run_path(script)["main"](["--ndjson-dir", str(raw), "--class-list", str(tmp_path / "list.txt"), "--target-dir", str(out),
                                    "--epsilon", "2.0", "--n-train", "3", "--n-valid", "2", "--n-test", "1"])
    want = []
    for r in records:
        if not r["recognized"]:
            continue
        lines = simplify.scale_to_255(simplify.quickdraw_lines(r["drawing"]))
        want.append(simplify.drawing_to_stroke3([l[ref.rdp_mask(l, 2.0) != 0] for l in lines]))
    assert len(want) == 6 and want[5].tolist() == [[0, 0, 0], [0, 0, 1]]
    with np.load(str(out / "thing.npz"), allow_pickle=True) as npz:
        got = list(npz["train"]) + list(npz["valid"]) + list(npz["test"])
        assert [len(npz[k]) for k in ("train", "valid", "test")] == [3, 2, 1]
    for g, w in zip(got, want):
        assert g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w)
    assert sum(len(w) for w in want) < sum(len(s[0]) for r in records for s in r["drawing"]) // 2


def test_chunk_script_with_simplification(tmp_path):
    target = tmp_path / "chunks"
    ref.run_chunk_script(target, "--simplify-epsilon", "2")
    stds, means = 0, 0
    for name in ("train_000.npz", "train_001.npz", "valid.npz", "test.npz"):
        with np.load(os.path.join(GOLDEN, "cut0", name), allow_pickle=True) as plain, np.load(str(target / name), allow_pickle=True) as got:
            want = [ref.simplify_stroke3(s, 2.0).astype(np.int16) for s in plain["x"]]
            assert len(got["x"]) == len(want) and np.array_equal(got["y"], plain["y"])
            assert all(g.dtype == np.int16 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got["x"], want))
            if name.startswith("train"):
                data = np.concatenate([w[:, :2] for w in want])
                assert data.dtype == np.int16
                assert got["std"].tobytes() == np.std(data).tobytes() and got["mean"].tobytes() == np.mean(data).tobytes()
                stds, means = stds + np.std(data), means + np.mean(data)
                assert sum(len(w) for w in want) < sum(len(s) for s in plain["x"])
    with np.load(str(target / "meta.npz")) as meta:
        assert meta["std"].tobytes() == np.asarray(stds / 2).tobytes() and meta["mean"].tobytes() == np.asarray(means / 2).tobytes()
