"""CPU tests of gradient clipping: the float64 / float32 restatement against answers worked by hand and against the Keras forms, the
rule of the settings, the host-only part of the C ABI (the segment plan) and the new model in the registry."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import clip_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_norms_worked_by_hand():
    flat = np.full(40, np.nan, dtype=np.float32)                 # whatever lies between the entries is never read
    ents = [R.entry(0, 1, 2), R.entry(4, 1, 1), R.entry(8, 2, 2, 8)]
    flat[0:2] = [3.0, 4.0]
    flat[4] = -12.0
    flat[8:10], flat[16:18] = [1.0, 2.0], [2.0, 4.0]             # a strided 2 x 2 view: rows at 8 and 16
    per, glob = R.norms(flat, ents)
    assert per.tolist() == [5.0, 12.0, 5.0]
    assert glob == np.sqrt(25.0 + 144.0 + 25.0)
    assert R.norms(flat, ents[:2])[1] == 13.0                    # 5-12-13
    assert R.norms(flat, ents[:2], grad_scale=0.5)[1] == 6.5     # grad_scale is a factor on the norms
    assert R.nonfinite(flat, ents) == 0


def test_scales_known_answers_and_boundaries():
    assert R.scale(5.0, 5.0) == np.float32(1.0)                  # norm == c: exactly 1
    assert R.scale(4.999, 5.0) == np.float32(1.0)
    assert R.scale(0.0, 5.0) == np.float32(1.0)                  # zero norm
    assert R.scale(10.0, 5.0) == np.float32(0.5)
    assert R.scale(3.0, 1.0) == np.float32(1.0) / np.float32(3.0) and R.scale(3.0, 1.0).dtype == np.float32
    assert R.scale(np.nextafter(np.float32(5.0), np.float32(6.0)), 5.0) < np.float32(1.0)
    g, per = R.scales(np.array([5.0, 12.0], np.float32), np.float32(13.0), "global", 6.5)
    assert g == np.float32(0.5) and per.tolist() == [1.0, 1.0]
    g, per = R.scales(np.array([5.0, 12.0], np.float32), np.float32(13.0), "per_variable", 6.0)
    assert g == np.float32(1.0) and per.tolist() == [1.0, 0.5]
    g, per = R.scales(np.array([5.0, 12.0], np.float32), np.float32(13.0), "none", 0.0)
    assert g == np.float32(1.0) and per.tolist() == [1.0, 1.0]


def test_clipvalue_and_skip_rule():
    g = np.array([-3.0, -0.5, 0.0, 0.25, 7.0], np.float32)
    assert R.swept_gradient(g, clipvalue=1.0).tolist() == [-1.0, -0.5, 0.0, 0.25, 1.0]
    assert R.swept_gradient(g, clipvalue=0.0).tolist() == g.tolist()
    assert R.swept_gradient(g, grad_scale=0.5, s=0.5).tolist() == (g * np.float32(0.25)).tolist()
    flat = np.array([1.0, np.inf, -np.inf, np.nan, 2.0], np.float32)
    assert R.nonfinite(flat, [R.entry(0, 1, 5)]) == 3 and R.nonfinite(flat, [R.entry(4, 1, 1)]) == 0
    assert R.skip(3, True) and not R.skip(3, False) and not R.skip(0, True)


def test_one_multiply_agrees_with_the_keras_forms_to_rounding():
    rng = np.random.RandomState(0)
    a, b = rng.randn(7, 5).astype(np.float32), (3.0 * rng.randn(11)).astype(np.float32)
    flat = np.concatenate([a.reshape(-1), np.zeros(1, np.float32), b])
    ents = [R.entry(0, 7, 5), R.entry(36, 1, 11)]
    per, glob = R.norms(flat, ents)
    for c in (0.5 * glob, 2.0 * glob):                           # active and inactive
        s, _ = R.scales(per.astype(np.float32), np.float32(glob), "global", c)
        for ours, keras in zip((a * s, b * s), R.keras_clip_by_global_norm([a, b], c)):
            # three float32 roundings on either side
            np.testing.assert_allclose(ours, keras, rtol=4 * 2.0 ** -24, atol=0)
    c = float(np.median(per))
    _, se = R.scales(per.astype(np.float32), np.float32(glob), "per_variable", c)
    for x, s in zip((a, b), se):
        np.testing.assert_allclose(x * s, R.keras_clip_by_norm(x, c), rtol=4 * 2.0 ** -24, atol=0)
    assert se.min() < 1.0 and se.max() == 1.0


def test_settings_rule_is_pure_and_refuses_two_modes():
    from sketchformer_amd import engine
    assert engine.check_gradient_clip() == (0, 0.0, 0.0)
    assert engine.check_gradient_clip(clipnorm=0.0, global_clipnorm=0, clipvalue=None) == (0, 0.0, 0.0)
    assert engine.check_gradient_clip(clipnorm=1.5) == (1, 1.5, 0.0)
    assert engine.check_gradient_clip(global_clipnorm=2.0) == (2, 2.0, 0.0)
    assert engine.check_gradient_clip(clipvalue=0.25) == (0, 0.0, 0.25)
    for kw in (dict(clipnorm=1.0, global_clipnorm=1.0), dict(clipnorm=1.0, clipvalue=1.0), dict(global_clipnorm=1.0, clipvalue=1.0),
               dict(clipnorm=1.0, global_clipnorm=1.0, clipvalue=1.0)):
        with pytest.raises(ValueError, match="at most one"):
            engine.check_gradient_clip(**kw)
    for bad in (-1.0, float("inf"), float("nan"), 1e39):
        for name in ("clipnorm", "global_clipnorm", "clipvalue"):
            with pytest.raises(ValueError, match=name):
                engine.check_gradient_clip(**{name: bad})


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def test_library_validates_the_settings_like_the_python_rule(lib):
    assert lib.skf_gradient_clip_validate(0, 0.0, 0.0) == 0
    assert lib.skf_gradient_clip_validate(1, 1.5, 0.0) == 0 and lib.skf_gradient_clip_validate(2, 2.0, 0.0) == 0
    assert lib.skf_gradient_clip_validate(0, 0.0, 0.25) == 0
    assert lib.skf_gradient_clip_validate(2, 1.0, 0.5) == -1 and b"at most one" in lib.skf_last_error()
    assert lib.skf_gradient_clip_validate(1, 1.0, 0.5) == -1
    assert lib.skf_gradient_clip_validate(3, 1.0, 0.0) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.skf_gradient_clip_validate(2, bad, 0.0) == -1 and b"threshold" in lib.skf_last_error()
    for bad in (-1.0, float("inf"), float("nan")):
        assert lib.skf_gradient_clip_validate(0, 0.0, bad) == -1 and b"clipvalue" in lib.skf_last_error()


def test_segment_plan_counts_and_limits(lib):
    """The plan is host work: chunk counts follow the fixed chunk size, and a bad entry is refused with a message."""
    from sketchformer_amd import ops, engine
    assert ops.SEGMENT_CHUNK == R.CHUNK
    ents = [R.entry(0, 1, 1), R.entry(4, 1, 3), R.entry(8, 5, 7), R.entry(44, 8, 12, 36), R.entry(56, 8, 12, 36),
            R.entry(400, 1, 2 * R.CHUNK + 5), R.entry(400 + 2 * R.CHUNK + 8, R.CHUNK, 1)]
    arr = ops._entry_array(ents)
    assert lib.skf_segment_plan_chunks(arr, len(ents)) == R.n_chunks(ents) == 1 + 1 + 1 + 1 + 1 + 3 + 1
    nbytes = lib.skf_segment_plan_bytes(len(ents), R.n_chunks(ents))
    assert nbytes > 0 and lib.skf_segment_plan_bytes(3, 2) == 0          # an entry has at least one chunk
    buf = (C.c_char * nbytes)()
    assert lib.skf_segment_plan_build(arr, len(ents), buf, nbytes) == 0
    assert lib.skf_segment_plan_build(arr, len(ents), buf, nbytes - 1) == -1
    head = np.frombuffer(buf, dtype=np.int32, count=3)
    assert head.tolist() == [len(ents), R.n_chunks(ents), R.CHUNK]
    assert lib.skf_segment_stats_floats(len(ents)) == 8 + 2 * len(ents)
    assert lib.skf_segment_norms_workspace_bytes(len(ents), R.n_chunks(ents)) > 0
    for bad in (R.entry(-4, 1, 1), R.entry(0, 0, 4), R.entry(0, 2, 4, 3), R.entry(0, 1 << 16, 1 << 15)):
        assert lib.skf_segment_plan_chunks(ops._entry_array([bad]), 1) == -1
        assert b"segment plan" in lib.skf_last_error()
    # the model's own table: every entry planned, and the clip workspace holds its stats words
    cfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
    entries = engine.param_entries(cfg)
    assert lib.skf_segment_plan_chunks(ops._entry_array(entries), len(entries)) == R.n_chunks(entries)
    assert lib.skf_model_clip_workspace_bytes(C.byref(cfg)) >= 4 * (8 + 2 * len(entries))


def test_registry_finds_the_clip_model_and_its_hparams():
    from sketchformer_amd import models
    G = json.load(open(os.path.join(HERE, "golden", "reference_goldens.json")))
    P = models.get_model_by_name("sketch-transformer-tf2")
    M = models.get_model_by_name("sketch-transformer-tf2-clip")
    assert issubclass(M, P) and M.name == "sketch-transformer-tf2-clip"
    five = dict(clipnorm=0.0, global_clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False, grad_report_every=0)
    assert M.specific_default_hparams().values() == {**P.specific_default_hparams().values(), **five}
    assert P.specific_default_hparams().values() == G["model_specific_defaults"]        # the parent's did not grow
    assert P.quick_metrics == G["model_attrs"]["quick_metrics"]
    assert M.quick_metrics == P.quick_metrics + ["grad_norm", "skipped_steps"] and M.slow_metrics == P.slow_metrics
    h = M.parse_hparams(base="batch_size=8", specific="global_clipnorm=0.5,skip_nonfinite=true,grad_report_every=10")
    assert (h.global_clipnorm, h.skip_nonfinite, h.grad_report_every, h.clipnorm) == (0.5, True, 10, 0.0)
    with pytest.raises(ValueError):
        P.parse_hparams(base=None, specific="global_clipnorm=0.5")
