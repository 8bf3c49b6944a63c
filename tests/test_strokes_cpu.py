"""The stroke-edit rule on the CPU: the restatement's own properties on integer-valued data, the list builders of
sketchformer_amd/strokes.py against hand-written lists, the workspace queries, the experiment's aggregates, and the
ink-preservation fixture that tests/test_gpu_strokes.py relies on."""
import numpy as np
import pytest

import align_reference as ar
import shape_reference as sr
import strokes_reference as st
from sketchformer_amd import strokes


@pytest.fixture(scope="module")
def ints():
    rng = np.random.RandomState(61)
    pool = [st.int_sketch(rng, [int(v) for v in rng.randint(1, 12, size=int(rng.randint(1, 7)))]) for _ in range(12)]
    pool.append(st.int_sketch(rng, [6]))                                       # one stroke
    pool.append(st.int_sketch(rng, [1, 1, 1]))
    return pool


def _positions(s):
    return np.cumsum(np.asarray(s)[:, :2], axis=0, dtype=np.float32)


# ---------------------------------------------------------------- the restatement
def test_identity_edit_returns_the_input_bits(ints):
    counts = [len(st.stroke_ranges(s)) for s in ints]
    out = st.edit(ints, range(len(ints)), [range(c) for c in counts])
    assert all(st.same_bits(a, b) for a, b in zip(out, ints))
    open_end = st.int_sketch(np.random.RandomState(1), [3, 4], lift_last=False)
    got = st.edit_one(open_end, [0, 1])
    assert st.same_bits(got[:, :2], open_end[:, :2]) and got[-1, 2] == 1 and open_end[-1, 2] == 0      # only that pen differs


def test_a_permutation_and_its_inverse_return_the_input(ints):
    rng = np.random.RandomState(62)
    for s in ints:
        c = len(st.stroke_ranges(s))
        p = rng.permutation(c)
        shuffled = st.edit_one(s, p)
        assert len(shuffled) == len(s) and len(st.stroke_ranges(shuffled)) == c
        assert st.same_bits(st.edit_one(shuffled, np.argsort(p)), s)


def test_reversing_twice_returns_the_input(ints):
    for s in ints:
        c = len(st.stroke_ranges(s))
        for order in (False, True):
            lists = strokes.reverse_lists([c], direction=True, order=order)[0]
            once = st.edit_one(s, lists)
            twice = st.edit_one(once, lists)
            assert twice.shape == s.shape and np.array_equal(twice, s)           # values (a sign flip may leave a -0)
            assert np.array_equal(np.abs(twice).view(np.int32), np.abs(s).view(np.int32))
    s = ints[0]
    c = len(st.stroke_ranges(s))
    back = st.edit_one(s, strokes.reverse_lists([c], order=True)[0])
    assert np.array_equal(_positions(back), _positions(s)[::-1])               # the drawing backwards in time: the same points


def test_backward_rows_flip_the_stored_sign_bits():
    s = np.array([[3, 4, 0], [0.0, -2, 0], [-0.0, 5, 1], [1, 1, 1]], np.float32)
    got = st.edit_one(s, [~0, 1])
    want = np.array([[3, 7, 0], [0.0, -5, 0], [-0.0, 2, 1], [1, 4, 1]], np.float32)
    assert st.same_bits(got, want)
    assert st.edit_one(s, [2, ~2, 5]).shape == (0, 3) and st.edit_one(None, [0]).shape == (0, 3)
    assert st.same_bits(st.edit_one(s, [7, 1, ~9, 1]), np.array([[4, 8, 1], [0, 0, 1]], np.float32))   # absent entries join


def test_table_of_the_restatement():
    s = [np.zeros((0, 3), np.float32), np.array([[1, 2, 0], [3, 4, 1], [5, 6, 0]], np.float32), np.array([[7, 8, 1]], np.float32)]
    ss, rows, ends = st.stroke_table(s)
    assert ss.tolist() == [0, 0, 2, 3] and rows.tolist() == [0, 2, 3, 4]
    assert ends.tolist() == [[1, 2, 4, 6], [9, 12, 9, 12], [7, 8, 7, 8]]


def test_leave_one_stroke_out_counts_owners_and_dropped(ints):
    counts = [len(st.stroke_ranges(s)) for s in ints]
    lists, owner, dropped = strokes.leave_one_out_lists(counts)
    assert len(lists) == sum(c for c in counts if c >= 2) == len(owner) == len(dropped)
    at = 0
    for i, c in enumerate(counts):
        if c < 2:
            continue
        for j in range(c):
            assert owner[at] == i and dropped[at] == j and lists[at].tolist() == [k for k in range(c) if k != j]
            v = st.edit_one(ints[i], lists[at])
            lo, hi = st.stroke_ranges(ints[i])[j]
            assert len(v) == len(ints[i]) - (hi - lo + 1) and len(st.stroke_ranges(v)) == c - 1
            at += 1
    assert at == len(lists)


# ---------------------------------------------------------------- the list builders
def test_list_builders_against_hand_written_lists():
    counts = [3, 1, 0, 4]
    as_lists = lambda ls: [np.asarray(l).tolist() for l in ls]                 # noqa: E731
    assert as_lists(strokes.identity_lists(counts)) == [[0, 1, 2], [0], [], [0, 1, 2, 3]]
    assert as_lists(strokes.reverse_lists(counts)) == [[-1, -2, -3], [-1], [], [-1, -2, -3, -4]]
    assert as_lists(strokes.reverse_lists(counts, order=True)) == [[-3, -2, -1], [-1], [], [-4, -3, -2, -1]]
    assert as_lists(strokes.reverse_lists(counts, direction=False, order=True)) == [[2, 1, 0], [0], [], [3, 2, 1, 0]]
    assert as_lists(strokes.keep_first_lists(counts, 2)) == [[0, 1], [0], [], [0, 1]]
    assert as_lists(strokes.keep_first_lists(counts, 0)) == [[], [], [], []]
    lists, owner, dropped = strokes.leave_one_out_lists(counts)
    assert as_lists(lists) == [[1, 2], [0, 2], [0, 1], [1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert owner.tolist() == [0, 0, 0, 3, 3, 3, 3] and dropped.tolist() == [0, 1, 2, 0, 1, 2, 3]
    rng = np.random.RandomState(5)
    assert as_lists(strokes.permutation_lists(counts, seed=5)) == [rng.permutation(c).tolist() for c in counts]
    assert as_lists(strokes.permutation_lists(counts, orders=[[2, 0, 1], [0], [], [3, 1, 0, 2]])) == [[2, 0, 1], [0], [], [3, 1, 0, 2]]
    with pytest.raises(ValueError):
        strokes.permutation_lists(counts, orders=[[0, 0, 1], [0], [], [0, 1, 2, 3]])
    with pytest.raises(ValueError):
        strokes.permutation_lists(counts, orders=[[0, 1, 2]])
    sel, sel_offsets = strokes.pack_selections([[0, -1], [], [5]])
    assert sel.dtype == np.int32 and sel.tolist() == [0, -1, 5] and sel_offsets.dtype == np.int64 and sel_offsets.tolist() == [0, 2, 2, 3]


def test_stroke_counts_on_the_host():
    data = [np.array([[1, 1, 0], [1, 1, 1], [2, 2, 0]], np.int16), np.zeros((0, 3), np.int16), np.array([[1, 1, 1]], np.float32),
            np.array([[1, 1, 2], [1, 1, 1], [0, 0, 1]], np.float32)]
    assert strokes.stroke_counts(data).tolist() == [2, 0, 1, 2]
    assert strokes.stroke_counts(data).tolist() == [len(st.stroke_ranges(s)) for s in data]
    with pytest.raises(IndexError):                                            # an empty sketch cannot be encoded; before the device
        strokes.leave_one_stroke_out(data)


# ---------------------------------------------------------------- the workspace queries
def test_workspace_queries():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    lib = _lib.load()
    q = lib.skf_stroke_table_workspace_bytes
    for P, N in ((0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3)):
        assert q(P, N) == 0, (P, N)
    sizes = [q(P, 7) for P in (1, 2, 63, 64, 65, 1000, 100000, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes) and q(1000, 7) <= q(1000, 7000)
    e = lib.skf_stroke_edit_workspace_bytes
    for P, N, M, Q in ((0, 1, 1, 1), (1 << 31, 1, 1, 1), (10, 0, 1, 1), (10, 1, 0, 1), (10, 1, -2, 1), (10, 1, 1, -1), (10, 1, 1, 1 << 31)):
        assert e(P, N, M, Q) == 0, (P, N, M, Q)
    assert e(10, 1, 1, 0) > 0                                                   # an edit that lists nothing is an edit
    sizes = [e(1000, 7, 5, Q) for Q in (0, 1, 63, 64, 65, 1000, 100000, (1 << 31) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] and all(s % 16 == 0 for s in sizes)
    assert sizes[-1] >= 16 * ((1 << 31) - 1)
    sizes = [e(1000, 7, M, 100) for M in (1, 64, 65, 100000, (1 << 31) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] and all(s % 16 == 0 for s in sizes)


# ---------------------------------------------------------------- the experiment's aggregates
def test_experiment_aggregates():
    from sketchformer_amd import experiments
    from sketchformer_amd.experiments.stroke_sensitivity import aggregate, aggregate_importance, cosine, format_table
    Exp = experiments.get_experiment_by_name("stroke-sensitivity")
    h = Exp.default_hparams()
    assert (h.set_type, h.n_sketches, h.n_permutations, h.seed, h.max_variants_per_batch) == ('test', 64, 4, 0, 4096)
    assert cosine([[1, 0], [1, 1], [0, 0]], [[2, 0], [1, -1], [1, 1]]).tolist() == [1.0, 0.0, 0.0]
    ctrl = np.array([0.5, 1.0])
    t = aggregate(('permutation', 'direction'), [np.array([[1.0, 0.5], [0.5, 0.0]]), np.array([1.0, 0.0])],
                  [np.array([[0.5, 0.5], [0.25, 0.75]]), np.array([0.5, 0.0])], ctrl,
                  [np.array([[0, 1], [1, 1]]), np.array([0, 0])], [np.ones((2, 2)), np.array([2.0, 4.0])],
                  [np.zeros((2, 2)), np.array([0.0, 1.0])])
    assert t['kind'].tolist() == ['permutation', 'direction']
    assert t['cosine'].tolist() == [0.5, 0.5] and t['p_true'].tolist() == [0.5, 0.25] and t['p_true_drop'].tolist() == [0.25, 0.5]
    assert t['class_changed'].tolist() == [0.75, 0.0] and t['dtw'].tolist() == [1.0, 3.0] and t['chamfer'].tolist() == [0.0, 0.5]
    with pytest.raises(ValueError):
        aggregate(('a',), [np.zeros(3)], [np.zeros(3)], ctrl, [np.zeros(3)], [np.zeros(3)], [np.zeros(3)])
    # strokes 0 .. 4 of a sketch of five, and both strokes of a sketch of two
    imp = aggregate_importance([0, 1, 2, 3, 4, 0, 1], [5, 5, 5, 5, 5, 2, 2], [0.5, 0.25, 0.125, 1.0, -1.0, 0.0, 0.5],
                               [0.05, 0.1, 0.2, 0.25, 0.4, 0.5, 0.75])
    assert imp['rank'].tolist() == ['first', 'second', 'third', 'later', 'last']
    assert imp['rank_importance'].tolist() == [0.25, 0.25, 0.125, 1.0, -0.25] and imp['rank_count'].tolist() == [2, 1, 1, 1, 2]
    assert imp['share_count'].tolist() == [2, 2, 2, 1] and imp['share_importance'].tolist() == [0.375, 0.5625, -0.5, 0.5]
    empty = aggregate_importance([], [], [], [])
    assert np.isnan(empty['rank_importance']).all() and empty['rank_count'].tolist() == [0] * 5
    text = format_table(t, imp)
    assert text.splitlines()[0].startswith("variant") and "permutation" in text and "last" in text and "10-25%" in text


# ---------------------------------------------------------------- the ink-preservation fixture of the GPU test
def test_ink_fixture_keeps_the_ink_and_changes_the_order():
    sketches, orders = st.ink_fixture()
    assert len(sketches) >= 4
    for s, order in zip(sketches, orders):
        assert np.array_equal(s, np.rint(s)) and np.abs(_positions(s)).max() < 2 ** 24
        c = len(st.stroke_ranges(s))
        assert sorted(order) == list(range(c)) and list(order) != list(range(c))
        xy, pen = _positions(s), s[:, 2]
        variants = {"permuted": st.edit_one(s, order), "direction": st.edit_one(s, strokes.reverse_lists([c])[0]),
                    "time": st.edit_one(s, strokes.reverse_lists([c], order=True)[0])}
        for name, v in variants.items():
            parts = sr.shape_ref(xy, pen, _positions(v), v[:, 2], 1)
            assert parts.tolist() == [0.0, 0.0, 0.0, 0.0], (name, parts)
            assert ar.dtw_ref(xy, _positions(v)) > 0, name
