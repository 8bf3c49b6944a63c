"""Gradient clipping in the train step (TrainEngine.set_gradient_clip -> skf_model_apply_gradients_clipped) against a TWIN engine:
same parameters, the first engine's gradient buffer COPIED into it pre-scaled in torch by the reported scale(s), then the plain
sweep - parameters and both moments must be the same bits.  iterations starts at 3000: the very first Keras update has lr 0."""
import json

import numpy as np
import pytest
import torch

import clip_reference as R

pytestmark = pytest.mark.gpu

KW = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
KW16 = dict(seq_len=40, d_model=128, num_heads=2, dff=256, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
B, START = 4, 3000
NORM_RTOL = 2.0 ** -23          # derivation in tests/test_gpu_gradnorm.py


def _mk(optimizer="Adam", use_graph=False, act_dtype="f32", kw=KW, batch=B):
    from sketchformer_amd import engine
    eng = engine.TrainEngine(engine.make_config(batch=batch, dropout_rate=0.0, use_graph=use_graph, optimizer=optimizer, seed=5,
                                                act_dtype=act_dtype, **kw), init_seed=1)
    eng.state[0] = START
    return eng


def _batch(kw=KW, batch=B, seed=3):
    from sketchformer_amd import synthetic
    return synthetic.token_batch(batch, kw["seq_len"], kw["vocab_size"], kw["n_classes"], seed=seed)


def _view(flat, e):
    return torch.as_strided(flat, (e["rows"], e["cols"]), (e["row_stride"], 1), e["offset"])


def _same(a, b):
    a.synchronize(); b.synchronize()
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("params", "adam_m", "adam_v"))


def _device_norms(eng, g):
    from sketchformer_amd import ops
    return ops.read_segment_stats(ops.segment_norms(g, ops.segment_plan(eng.entries, eng.device)), len(eng.entries))


def _settings(kind, eng, g):
    """the clip settings of a case, from the norms of the gradient at hand"""
    base = _device_norms(eng, g)
    if kind == "global":
        return dict(global_clipnorm=0.5 * base["global_norm"])
    if kind == "global-inactive":
        return dict(global_clipnorm=2.0 * base["global_norm"])
    if kind == "per-variable":
        return dict(clipnorm=float(np.median(base["norms"])))
    if kind == "clipvalue":
        return dict(clipvalue=float(g.abs().median()))
    return dict(monitor=True)


def _prescaled(eng, g, settings, stats):
    """the gradient the clipped sweep saw, made in torch from the engine's reported scales"""
    g = g.clone()
    if "global_clipnorm" in settings:
        g *= float(np.float32(stats["scale"]))
    elif "clipnorm" in settings:
        for e in eng.entries:
            v = _view(g, e)
            v.copy_(v * float(np.float32(stats["scales"][e["name"]])))
    elif "clipvalue" in settings:
        cv = float(np.float32(settings["clipvalue"]))
        g.clamp_(-cv, cv)
    return g


def _step_against_twin(eng, twin, settings_kind, x, y, bucketed=None, configure=True):
    eng.forward_backward(x, None, y)
    twin.forward_backward(x, None, y)                  # (its prologue: the step's lr / alpha; its own gradient is overwritten below)
    g = eng.grads.clone()
    if configure:
        settings = _settings(settings_kind, eng, g)
        eng.set_gradient_clip(**settings)
        eng._settings = settings
    eng.apply_gradients(bucketed=bucketed)
    stats = eng.gradient_stats()
    twin.grads.copy_(_prescaled(eng, g, eng._settings, stats))
    twin.apply_gradients()
    return stats, g


def test_reported_norms_match_the_restatement_and_monitoring_changes_nothing():
    eng, twin = _mk(), _mk()
    x, y = _batch()
    eng.forward_backward(x, None, y)
    G = eng.state_dict_numpy("grads")
    eng.set_gradient_clip(monitor=True)
    eng.apply_gradients()
    st = eng.gradient_stats()
    total = 0.0
    for name, g in G.items():
        ss = float(np.sum(np.square(g.astype(np.float64))))
        total += ss
        want = np.sqrt(ss)
        assert abs(st["norms"][name] - want) <= NORM_RTOL * want, (name, st["norms"][name], want)
        assert st["scales"][name] == 1.0
    want = np.sqrt(total)
    print("global norm %.9g, float64 %.17g" % (st["global_norm"], want))
    assert st["global_norm"] > 0 and abs(st["global_norm"] - want) <= NORM_RTOL * want
    assert st["scale"] == 1.0 and st["nonfinite"] == 0 and not st["skipped"] and st["skipped_total"] == 0
    twin.train_step(x, y)                                # an engine that was never configured
    assert _same(eng, twin) and eng.iterations == twin.iterations == START + 1
    rep = eng.gradient_report()
    P = eng.state_dict_numpy("params")
    for name, row in rep["variables"].items():
        wn = np.sqrt(np.sum(np.square(P[name].astype(np.float64))))
        assert row["grad_norm"] == st["norms"][name] and abs(row["weight_norm"] - wn) <= NORM_RTOL * wn
        assert row["ratio"] == (row["grad_norm"] / row["weight_norm"] if row["weight_norm"] else (float("inf") if row["grad_norm"] else 0.0))
    assert rep["global_norm"] == st["global_norm"] and rep["weight_global_norm"] > 0


@pytest.mark.parametrize("kind,optimizer,use_graph,bucketed", [
    ("global", "Adam", False, None), ("global-inactive", "Adam", False, None), ("per-variable", "Adam", False, None),
    ("clipvalue", "Adam", False, None), ("global", "SGD", False, None), ("per-variable", "SGD", False, None),
    ("global", "Adam", True, None), ("per-variable", "Adam", True, None), ("clipvalue", "SGD", True, None),
    ("global", "Adam", False, True)])
def test_clipped_step_equals_the_plain_sweep_over_a_prescaled_gradient(kind, optimizer, use_graph, bucketed):
    eng, twin = _mk(optimizer, use_graph), _mk(optimizer, use_graph)
    x, y = _batch()
    before = eng.params.clone()
    stats, g = _step_against_twin(eng, twin, kind, x, y, bucketed=bucketed)
    assert _same(eng, twin), (kind, optimizer, use_graph, bucketed)
    assert eng.iterations == twin.iterations == START + 1
    assert not torch.equal(eng.params, before)                                   # lr != 0: the step moved the weights
    assert stats["nonfinite"] == 0 and not stats["skipped"] and stats["skipped_total"] == 0
    if kind == "global":
        assert stats["scale"] == float(R.scale(stats["global_norm"], eng._settings["global_clipnorm"])) and 0.49 < stats["scale"] < 0.51
    elif kind == "global-inactive":
        assert stats["scale"] == 1.0
        plain = _mk(optimizer, use_graph)                                           # bit-equal to an unconfigured engine
        plain.forward_backward(x, None, y)
        plain.grads.copy_(g)
        plain.apply_gradients()
        assert _same(eng, plain)
    elif kind == "per-variable":
        s = np.array(list(stats["scales"].values()), np.float32)
        assert stats["scale"] == 1.0 and s.min() < 1.0 and s.max() == 1.0 and 0.2 < (s < 1.0).mean() < 0.8
        c = np.float32(eng._settings["clipnorm"])
        assert all(np.float32(stats["scales"][n]) == R.scale(stats["norms"][n], c) for n in stats["norms"])
    # a second step through the same (captured or eager) sequence, thresholds unchanged
    x2, y2 = _batch(seed=4)
    _step_against_twin(eng, twin, kind, x2, y2, bucketed=bucketed, configure=False)
    assert _same(eng, twin) and eng.iterations == twin.iterations == START + 2


@pytest.mark.parametrize("use_graph", [False, True])
def test_nonfinite_gradient_skips_the_step_and_the_next_clean_step_is_normal(use_graph):
    eng, twin = _mk(use_graph=use_graph), _mk(use_graph=use_graph)
    x, y = _batch()
    eng.forward_backward(x, None, y)
    c = 0.5 * _device_norms(eng, eng.grads.clone())["global_norm"]
    eng.set_gradient_clip(global_clipnorm=c, skip_nonfinite=True)
    eng._settings = dict(global_clipnorm=c)
    e = [e for e in eng.entries if e["rows"] > 1 and e["row_stride"] == e["cols"]][3]      # some contiguous matrix: row 1, column 1
    eng.grads[e["offset"] + e["cols"] + 1] = float("inf")
    held = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    eng.apply_gradients()
    st = eng.gradient_stats()
    assert st["nonfinite"] == 1 and st["skipped"] and st["skipped_total"] == 1
    assert all(torch.equal(a, b) for a, b in zip(held, (eng.params, eng.adam_m, eng.adam_v)))
    assert eng.iterations == START                                                  # a skipped step is no optimizer iteration
    stats, _ = _step_against_twin(eng, twin, "global", x, y, configure=False)
    assert _same(eng, twin) and eng.iterations == twin.iterations == START + 1
    assert not stats["skipped"] and stats["nonfinite"] == 0 and stats["skipped_total"] == 1 and stats["scale"] < 1.0


def test_configure_then_unconfigure_is_an_unconfigured_engine():
    from sketchformer_amd import _lib
    eng, plain = _mk(use_graph=True), _mk(use_graph=True)
    with pytest.raises(ValueError, match="at most one"):
        eng.set_gradient_clip(clipnorm=1.0, global_clipnorm=1.0)
    with pytest.raises(_lib.SkfError):
        eng.gradient_stats()
    eng.set_gradient_clip(global_clipnorm=1e-3, skip_nonfinite=True)
    eng.set_gradient_clip()
    assert eng._clip is None
    for s in range(3):
        x, y = _batch(seed=10 + s)
        eng.train_step(x, y)
        plain.train_step(x, y)
    assert _same(eng, plain) and eng.iterations == plain.iterations == START + 3


def test_bf16_step_is_clipped_and_its_weight_images_follow():
    eng, twin = _mk(act_dtype="bf16", kw=KW16, batch=6), _mk(act_dtype="bf16", kw=KW16, batch=6)
    x, y = _batch(KW16, 6)
    stats, _ = _step_against_twin(eng, twin, "global", x, y)
    assert stats["scale"] < 1.0 and _same(eng, twin)
    eng.forward(x)
    twin.forward(x)
    eng.synchronize(); twin.synchronize()
    assert torch.equal(eng.buffer("logits"), twin.buffer("logits"))


SMALL = "num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"
DATA = "max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"


def test_plugin_model_reports_gradient_norms(tmp_path):
    from sketchformer_amd import models, dataloaders
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams(DATA), None)
    Model = models.get_model_by_name("sketch-transformer-tf2-clip")
    hps = Model.parse_hparams(base="batch_size=8,num_epochs=1,log_every=100", specific=SMALL + ",global_clipnorm=0.25,grad_report_every=1")
    model = Model(hps, dataset, str(tmp_path), "c0")
    it = dataset.batch_iterator("train", 8, False)
    results = [model.train_on_batch(next(it)) for _ in range(3)]
    last = dict(results[-1])
    assert last["grad_norm"] > 0 and last["skipped_steps"] == 0 and np.isfinite(last["total_loss"])
    assert set(last) == {"recon_loss", "recon_acc", "class_loss", "class_acc", "total_loss", "grad_norm", "skipped_steps"}
    lines = [json.loads(ln) for ln in open(tmp_path / "sketch-transformer-tf2-clip-c0" / "grad_norms.jsonl")]
    assert len(lines) == 3 and [ln["step"] for ln in lines] == [1, 2, 3]
    for ln in lines:
        assert set(ln["grad_norms"]) == set(ln["weight_norms"]) == set(model.trainable_variables)
        assert ln["grad_norm"] > 0 and 0 < ln["scale"] <= 1.0 and ln["skipped_steps"] == 0
    assert lines[-1]["grad_norm"] == last["grad_norm"]
    # the parent model's mapping did not grow
    Parent = models.get_model_by_name("sketch-transformer-tf2")
    parent = Parent(Parent.parse_hparams(base="batch_size=8,num_epochs=1,log_every=100", specific=SMALL), dataset, str(tmp_path), "p0")
    assert set(parent.train_on_batch(next(it))) == {"recon_loss", "recon_acc", "class_loss", "class_acc", "total_loss"}
    assert sorted(parent.quick_metrics) == sorted(["recon_loss", "recon_acc", "class_loss", "class_acc", "total_loss"])
