"""Device augmentation, the parts that need no GPU: the one-call draw against the host's interleaved draws, the restated rule
against the host, the workspace query, the empty-sketch error - and the three wrong-on-purpose variants that give
tests/test_gpu_augment.py its teeth, asserted here on the CPU so that the GPU tests cannot pass by accident."""
import numpy as np
import pytest

import augment_reference as aug
from preprocess_reference import host_loader
from sketchformer_amd import preprocess


def test_one_call_draws_the_interleaved_stream():
    """np.random.random(size=2 N + P) is the stream of the per-sketch calls: (), (), (size=n) for every sketch in turn."""
    sketches = aug.sweep_pool()[:300] + [np.zeros((0, 3), np.int16), aug.sketch(np.random.RandomState(1), 9)]
    np.random.seed(4321)
    one = np.random.random(size=aug.n_draws(sketches))
    after_one = np.random.random()
    np.random.seed(4321)
    parts = []
    for s in sketches:
        parts += [[np.random.random()], [np.random.random()], np.random.random(size=len(s))]
    assert np.array_equal(one, np.concatenate(parts)) and after_one == np.random.random()
    # and the host under a seed is the host under the replayed one-call stream
    loader = host_loader(use_continuous_data=True, augment_stroke_prob=0.3)
    np.random.seed(4321)
    want = [loader._augment_sketch(np.array(np.clip(s, -1000, 1000), dtype=np.float32)) for s in sketches]
    got = aug.host_augment(sketches, one, 0.1, 0.3)
    assert aug.n_differing(got, [np.asarray(w, np.float32).reshape(-1, 3) for w in want]) == 0
    assert got[-2].shape == (0, 3)                                   # the empty sketch took its two draws and gave no row


@pytest.mark.parametrize("prob", [0.1, 0.9, 1.0])
@pytest.mark.parametrize("clamp", [True, False])
def test_the_restated_rule_is_the_host(prob, clamp):
    sketches = aug.sweep_pool()[:130]
    rnd = np.random.RandomState(8).random_sample(aug.n_draws(sketches))
    want = aug.host_augment(sketches, rnd, 0.1, prob, clamp=clamp)
    assert aug.n_differing(aug.restate_all(sketches, rnd, 0.1, prob, clamp=clamp), want) == 0
    assert sum(len(w) for w in want) < sum(len(s) for s in sketches)


def test_the_first_droppable_point_is_index_3():
    """Sketches that end in a lift, every draw 0, prob = 1: lengths 1 - 4 stay, 5 and 6 shrink to 4 rows."""
    rng = np.random.RandomState(2)
    for n in range(1, 7):
        s = aug.sketch(rng, n, pen="last")
        (got,) = aug.host_augment([s], np.zeros(2 + n), 0.0, 1.0)
        assert len(got) == min(n, 4), n
        if n <= 4:
            assert np.array_equal(got, s.astype(np.float32))
        else:                                                        # (small integers: the merged sums are exact)
            assert np.array_equal(got[:2], s[:2].astype(np.float32)) and got[3].tolist() == s[-1].tolist()
            assert got[2].tolist() == s[2:n - 1].sum(0).tolist()


def test_fixture_a_the_order_of_the_adds_matters():
    sketches, rnd, e, prob = aug.order_fixture()
    want = aug.host_augment(sketches, rnd, e, prob)
    assert aug.n_differing(aug.restate_all(sketches, rnd, e, prob), want) == 0
    assert aug.n_differing(aug.restate_all(sketches, rnd, e, prob, sum_first=True), want) >= 1


def test_fixture_b_the_draw_is_compared_in_float64():
    sketches, rnd, e, prob = aug.threshold_fixture()
    want = aug.host_augment(sketches, rnd, e, prob)
    assert [len(w) for w in want] == [5, 5]                          # the point at index 3 is dropped
    assert aug.n_differing(aug.restate_all(sketches, rnd, e, prob), want) == 0
    wrong = aug.restate_all(sketches, rnd, e, prob, fp32_draws=True)
    assert [len(w) for w in wrong] == [6, 6] and aug.n_differing(wrong, want) >= 1


def test_fixture_c_the_scale_factors_are_float64():
    sketches, rnd, e, prob = aug.factor_fixture()
    want = aug.host_augment(sketches, rnd, e, prob)
    assert [len(w) for w in want] == [7] * 32                        # nothing dropped: only the factors act
    assert aug.n_differing(aug.restate_all(sketches, rnd, e, prob), want) == 0
    assert aug.n_differing(aug.restate_all(sketches, rnd, e, prob, fp32_factors=True), want) >= 1


def test_workspace_query():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    q = _lib.load().skf_sketch_augment_workspace_bytes
    for P, N in ((0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3)):
        assert q(P, N) == 0, (P, N)
    sizes = [q(P, 7) for P in (1, 2, 63, 64, 65, 1000, 100000, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= (1 << 31) - 1                                # a keep byte per point
    assert q(1000, 100000) >= 4 * 100000                             # and a count per sketch


def test_encode_chunk_refuses_an_empty_sketch_before_the_device(monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch.cuda, "Stream", boom)
    data = [np.array([[1, 2, 0], [3, 4, 1]], np.int16), np.zeros((0, 3), np.int16)]
    hps = host_loader(use_continuous_data=True).hps
    np.random.seed(5)
    with pytest.raises(IndexError):
        preprocess.encode_chunk(data, hps, None, augment=True)
    after = np.random.random()
    np.random.seed(5)
    assert after == np.random.random()                               # and before a draw was taken

