"""Device path flattening against the host restatement of tests/flatten_reference.py (tests/test_flatten_cpu.py asserts the
restatement's facts on the CPU).  Everything is equality on bit patterns - rows, offsets, shapes - there are no tolerances."""
import numpy as np
import pytest
import torch

import flatten_reference as fr
import resample_reference as rr
import simplify_reference as ref
from sketchformer_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 0.25


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # (a copy: the shared references are read-only)


def _flatten(ctrl, kind, offsets, tol):
    out_xy, out_offsets = ops.path_flatten(_dev(ctrl), _dev(kind), _dev(offsets), tol)
    assert out_xy.dtype == torch.float32 and out_xy.dim() == 2 and out_xy.shape[1] == 2 and out_xy.is_contiguous()
    assert out_offsets.dtype == torch.int64 and tuple(out_offsets.shape) == (len(offsets),)
    return out_xy.cpu().numpy(), out_offsets.cpu().numpy()


def _check(ctrl, kind, offsets, tol, want=None):
    got_xy, got_offsets = _flatten(ctrl, kind, offsets, tol)
    want_xy, want_offsets = fr.pack(fr.flatten(ctrl, kind, offsets, tol) if want is None else want)
    assert np.array_equal(got_offsets, want_offsets)
    assert fr.same_bits(got_xy, want_xy)
    return got_xy, got_offsets


@pytest.fixture(scope="module")
def batch():
    """about 2 000 short subpaths, every tenth segment a line, and the restatement's rows of each"""
    rng = np.random.RandomState(53)
    lengths = rng.randint(1, 5, size=2 * ref.OFFSETS_SCAN_BLOCK + 5)
    ctrl, kind, offsets = fr.random_subpaths(lengths.tolist(), seed=54, line_every=10)
    for a in (ctrl, kind, offsets):
        a.setflags(write=False)
    return ctrl, kind, offsets, fr.flatten(ctrl, kind, offsets, TOL)


# ---------------------------------------------------------------- ops.path_flatten
@pytest.mark.parametrize("segments", [1, 63, 64, 65, 200])
def test_subpath_lengths_around_a_wave(segments):
    ctrl, kind, offsets = fr.random_subpaths([segments, 3], seed=60 + segments)
    _, got = _check(ctrl, kind, offsets, TOL)
    assert got[1] > 5 * segments                                             # curves, not lines: well above one row a segment


def test_piece_counts_around_a_wave_and_at_the_ceiling():
    wanted = [1, 2, 63, 64, 65, fr.MAX_N]
    straight = np.array([(0, 0), (10, 20), (20, 40), (30, 60)], np.float64)
    ctrl = np.stack([straight] + [fr.bump(n, TOL) for n in wanted[1:]])
    kind = np.ones(len(ctrl), np.int32)
    assert fr.pieces(ctrl, kind, TOL).tolist() == wanted
    # each as a subpath of its own, then all of them as one subpath: row counts 1 + n, and 1 + the sum
    _, offsets = _check(ctrl, kind, np.arange(len(ctrl) + 1), TOL)
    assert np.diff(offsets).tolist() == [n + 1 for n in wanted]
    _, offsets = _check(ctrl, kind, np.array([0, len(ctrl)]), TOL)
    assert offsets.tolist() == [0, 1 + sum(wanted)]
    # the ceiling holds whatever the curve: a second difference far beyond 4096^4 c, and a NaN
    huge = np.array([(0, 0), (1e9, 1e9), (-1e9, 1e9), (0, 0)], np.float64)
    nan = np.array([(0, 0), (1, 1), (2, np.nan), (3, 0)], np.float64)
    _, offsets = _check(huge[None], np.ones(1, np.int32), np.arange(2), TOL)
    assert offsets.tolist() == [0, fr.MAX_N + 1]
    xy, offsets = _flatten(nan[None], np.ones(1, np.int32), np.arange(2), TOL)
    want = fr.flatten_subpath(nan[None], [1], TOL)
    assert offsets.tolist() == [0, fr.MAX_N + 1] and xy[-1].tolist() == [3, 0]
    assert fr.same_bits(xy[:, 0], want[:, 0]) and np.isnan(xy[1:-1, 1]).all()  # (the bits of a NaN are nobody's contract)


def test_lines_only_and_mixed_kinds():
    ctrl, kind, offsets = fr.random_subpaths([7, 70, 1], seed=70)
    lines = np.zeros_like(kind)
    xy, got = _check(ctrl, lines, offsets, TOL)
    assert got.tolist() == [0, 8, 79, 81]                                    # a line is one row, p1 and p2 play no part
    assert fr.same_bits(xy[1:8], ctrl[:7, 3].astype(np.float32))
    mixed = kind.copy()
    mixed[::3], mixed[1::7] = 0, 2                                           # a kind other than 0 or 1 is a line
    _, got_mixed = _check(ctrl, mixed, offsets, TOL)
    assert 81 < got_mixed[-1] < _check(ctrl, kind, offsets, TOL)[1][-1]


def test_empty_subpaths_in_front_in_the_middle_and_at_the_end():
    ctrl, kind, _ = fr.random_subpaths([9], seed=71)
    offsets = np.array([0, 0, 0, 4, 4, 4, 9, 9, 9], np.int64)
    _, got = _check(ctrl, kind, offsets, TOL)
    rows = np.diff(got)
    assert (rows[[0, 1, 3, 4, 6, 7]] == 0).all() and (rows[[2, 5]] > 5).all()
    # one subpath, and one empty subpath alone
    _check(ctrl, kind, np.array([0, 9]), TOL)
    xy, got = _flatten(ctrl, kind, np.array([4, 4]), TOL)
    assert xy.shape == (0, 2) and got.tolist() == [0, 0]


@pytest.mark.parametrize("S", [1, 64, ref.OFFSETS_SCAN_BLOCK + 1, 2 * ref.OFFSETS_SCAN_BLOCK + 5])
def test_batches_up_to_two_thousand_subpaths(batch, S):
    ctrl, kind, offsets, want = batch
    G = int(offsets[S])
    _check(ctrl[:G], kind[:G], offsets[:S + 1], TOL, want=want[:S])


@pytest.mark.parametrize("tol", [0.05, 1.0, 1e-3, 64.0])
def test_other_tolerances(batch, tol):
    ctrl, kind, offsets, _ = batch
    G = int(offsets[40])
    _check(ctrl[:G], kind[:G], offsets[:41], tol)


def test_offsets_outside_the_segments_are_clamped():
    """Negative, past the end, descending: the clamp to [0, G] defines the answer - segments 0 .. 5, 6 .. 9, nothing."""
    ctrl, kind, _ = fr.random_subpaths([10], seed=72)
    offsets = np.array([-5, 6, 12, 8], np.int64)
    want = [fr.flatten_subpath(ctrl[:6], kind[:6], TOL), fr.flatten_subpath(ctrl[6:], kind[6:], TOL), np.zeros((0, 2), np.float32)]
    _check(ctrl, kind, offsets, TOL, want=want)


def test_inputs_are_left_alone_and_two_calls_agree(batch):
    ctrl, kind, offsets, want = batch
    G = int(offsets[300])
    c_d, k_d, o_d = _dev(ctrl[:G]), _dev(kind[:G]), _dev(offsets[:301])
    first = ops.path_flatten(c_d, k_d, o_d, TOL)
    again = ops.path_flatten(c_d, k_d, o_d, TOL)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    assert fr.same_bits(first[0].cpu().numpy(), fr.pack(want[:300])[0])
    assert np.array_equal(c_d.cpu().numpy().view(np.int64), ctrl[:G].view(np.int64))
    assert np.array_equal(k_d.cpu().numpy(), kind[:G]) and np.array_equal(o_d.cpu().numpy(), offsets[:301])
    # a subpath's rows do not depend on the rest of the batch
    lo, hi = int(offsets[120]), int(offsets[121])
    alone = ops.path_flatten(c_d[lo:hi], k_d[lo:hi], _dev(np.array([0, hi - lo])), TOL)[0]
    assert fr.same_bits(alone.cpu().numpy(), want[120])
    only_offsets = ops.path_flatten_offsets(c_d, k_d, o_d, TOL)
    assert torch.equal(only_offsets, first[1])


def test_the_result_feeds_the_simplification_and_the_resampling_unchanged(batch):
    ctrl, kind, offsets, want = batch
    G = int(offsets[200])
    xy, out_offsets = ops.path_flatten(_dev(ctrl[:G]), _dev(kind[:G]), _dev(offsets[:201]), TOL)
    keep = ops.rdp_keep(xy, out_offsets, 1.5).cpu().numpy()
    assert np.array_equal(keep, ref.masks(want[:200], 1.5))
    assert 2 * 200 <= keep.sum() < 0.8 * len(keep)                            # the curve samples are what RDP is there to thin out
    res_xy, res_offsets = ops.polyline_resample(xy, out_offsets, 4.0)
    want_xy, want_offsets = rr.pack(rr.resample_all(want[:200], 4.0))
    assert np.array_equal(res_offsets.cpu().numpy(), want_offsets) and rr.same_bits(res_xy.cpu().numpy(), want_xy)
    dense = ops.polyline_resample_n(xy, out_offsets, 16)
    assert rr.same_bits(dense.cpu().numpy(), np.stack([rr.resample_n(w, 16) for w in want[:200]]))


# ---------------------------------------------------------------- the C ABI
def _abi():
    lib = _lib.load()
    ctrl, kind, offsets = fr.random_subpaths([3, 2], seed=73, line_every=4)
    want = fr.flatten(ctrl, kind, offsets, TOL)
    rows = sum(len(w) for w in want)
    st = {"lib": lib, "ctrl": _dev(ctrl), "kind": _dev(kind), "offsets": _dev(offsets),
          "out_offsets": torch.full((3,), -7, dtype=torch.int64, device=DEV),
          "out": torch.full((rows + 8, 2), -7.0, dtype=torch.float32, device=DEV)}
    st["ws_bytes"] = lib.skf_path_flatten_workspace_bytes(5, 2)
    assert st["ws_bytes"] > 0
    st["ws"] = torch.zeros(st["ws_bytes"] + 64, dtype=torch.uint8, device=DEV)
    st["want"], st["rows"], st["first"] = np.concatenate(want), rows, len(want[0])
    return st


def test_out_rows_is_a_capacity():
    st = _abi()
    lib, p = st["lib"], {k: st[k].data_ptr() for k in ("ctrl", "kind", "offsets", "out_offsets", "out", "ws")}
    assert lib.skf_path_flatten_count(p["ctrl"], p["kind"], 5, p["offsets"], 2, TOL, p["out_offsets"], p["ws"], st["ws_bytes"], None) == 0
    torch.cuda.synchronize()
    rows, first = st["rows"], st["first"]
    assert st["out_offsets"].tolist() == [0, first, rows] and (st["out"] == -7).all() and first > 10 and rows - first > 3
    for cap in (first + 3, first, first // 2, 1):                                    # inside the second subpath, between the two, inside the first
        st["out"].fill_(-7.0)
        assert lib.skf_path_flatten_emit(p["ctrl"], p["kind"], 5, p["offsets"], 2, TOL, p["out_offsets"], p["out"], cap, p["ws"],
                                         st["ws_bytes"], None) == 0
        torch.cuda.synchronize()
        got = st["out"].cpu().numpy()
        assert fr.same_bits(got[:cap], st["want"][:cap]) and (got[cap:] == -7).all(), cap
    st["out"].fill_(-7.0)
    assert lib.skf_path_flatten_emit(p["ctrl"], p["kind"], 5, p["offsets"], 2, TOL, p["out_offsets"], p["out"], rows + 8, p["ws"],
                                     st["ws_bytes"], None) == 0
    torch.cuda.synchronize()
    got = st["out"].cpu().numpy()
    assert fr.same_bits(got[:rows], st["want"]) and (got[rows:] == -7).all()  # rows no subpath owns stay as they were


def test_argument_limits_are_refused_with_their_message():
    st = _abi()
    lib = st["lib"]
    base = {k: st[k].data_ptr() for k in ("ctrl", "kind", "offsets", "out_offsets", "out", "ws")}

    def count(G=5, S=2, tol=TOL, ws_bytes=st["ws_bytes"], shift=None, null=None, **_):
        p = dict(base)
        if shift:
            p[shift[0]] += shift[1]
        if null:
            p[null] = None
        return lib.skf_path_flatten_count(p["ctrl"], p["kind"], G, p["offsets"], S, tol, p["out_offsets"], p["ws"], ws_bytes, None)

    def emit(G=5, S=2, tol=TOL, out_rows=st["rows"], ws_bytes=st["ws_bytes"], shift=None, null=None, **_):
        p = dict(base)
        if shift:
            p[shift[0]] += shift[1]
        if null:
            p[null] = None
        return lib.skf_path_flatten_emit(p["ctrl"], p["kind"], G, p["offsets"], S, tol, p["out_offsets"], p["out"], out_rows, p["ws"],
                                         ws_bytes, None)

    shared = [(dict(S=0), "S must be at least 1"), (dict(S=-1), "S must be at least 1"), (dict(G=0), "G must be in"),
              (dict(G=1 << 31), "G must be in"), (dict(ws_bytes=8), "workspace too small"),
              (dict(ws_bytes=st["ws_bytes"] - 1), "workspace too small"), (dict(shift=("ctrl", 4)), "aligned"),
              (dict(shift=("kind", 2)), "aligned"), (dict(shift=("offsets", 4)), "aligned"), (dict(shift=("ws", 8)), "aligned"),
              (dict(null="ctrl"), "null pointer"), (dict(null="kind"), "null pointer"), (dict(null="offsets"), "null pointer"),
              (dict(null="ws"), "null pointer")]
    tols = [(dict(tol=t), "tol must be finite and above 0") for t in (0.0, -1.0, float("nan"), float("inf"))]
    cases = [(count, shared + tols + [(dict(shift=("out_offsets", 4)), "8-byte aligned"), (dict(null="out_offsets"), "8-byte aligned")]),
             (emit, shared + tols + [(dict(shift=("out_offsets", 4)), "8-byte aligned"), (dict(shift=("out", 4)), "8-byte aligned"),
                                     (dict(null="out"), "8-byte aligned"), (dict(out_rows=0), "out_rows must be in"),
                                     (dict(out_rows=-1), "out_rows must be in"), (dict(out_rows=1 << 31), "out_rows must be in")])]
    for fn, bads in cases:
        for bad, text in bads:
            assert fn(**bad) == -1, (fn.__name__, bad)
            message = lib.skf_last_error().decode()
            assert text in message and ("skf_path_flatten_" + fn.__name__) in message, (bad, message)
    assert lib.skf_path_flatten_workspace_bytes(0, 1) == 0 and lib.skf_path_flatten_workspace_bytes(1 << 31, 1) == 0
    assert lib.skf_path_flatten_workspace_bytes(5, 0) == 0
    torch.cuda.synchronize()
    assert (st["out"] == -7).all() and (st["out_offsets"] == -7).all()       # nothing was launched
    assert count() == 0 and emit() == 0 and count(tol=1e-300) == 0 and count(tol=1e300) == 0
    torch.cuda.synchronize()
    # the wrappers refuse on the host
    ctrl, kind, offsets = st["ctrl"], st["kind"], st["offsets"]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol must be finite and above 0"):
            ops.path_flatten(ctrl, kind, offsets, bad)
    with pytest.raises(TypeError, match="ctrl must be a contiguous float64 tensor of shape"):
        ops.path_flatten(ctrl.float(), kind, offsets, TOL)
    with pytest.raises(TypeError, match="ctrl must be"):
        ops.path_flatten(ctrl.reshape(-1, 8), kind, offsets, TOL)
    with pytest.raises(TypeError, match="ctrl must be"):
        ops.path_flatten(ctrl.new_zeros(5, 4, 4)[:, :, :2], kind, offsets, TOL)        # not contiguous
    with pytest.raises(TypeError, match="kind must be a contiguous int32 tensor"):
        ops.path_flatten(ctrl, kind.long(), offsets, TOL)
    with pytest.raises(TypeError, match="kind must be"):
        ops.path_flatten(ctrl, kind[:4], offsets, TOL)
    with pytest.raises(TypeError, match="path_offsets must be a contiguous int64 tensor"):
        ops.path_flatten_offsets(ctrl, kind, offsets.to(torch.int32), TOL)
    with pytest.raises(ValueError, match="at least one subpath"):
        ops.path_flatten(ctrl, kind, offsets[:1], TOL)
    with pytest.raises(_lib.SkfError):
        ops.path_flatten(ctrl.cpu(), kind, offsets, TOL)
