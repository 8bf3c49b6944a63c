"""The launches of the two-stream train step that run on the side stream although they are not weight gradients: the class head's
forward and its cross-entropy (in front of the cross-attention K|V projections), the step-metrics launch (behind the output layer's
weight-gradient group) and the decoder embedding gradient (in front of decoder layer 0's group).  Every one of them computes what it
computed on the main stream, so each test here asks for bit equality: between two engines from one seed (a missing cross-stream
dependency shows up as a difference), against the one-stream step where the two run the same arithmetic, and between a host that
synchronises after every step and one that never does.  Shapes of test_two_stream_step_is_deterministic_in_every_model_structure:
16 x 50 tokens, d = 128, dff = 512, 8 heads, 2 layers - the smallest model with a held weight-gradient group and a deferred K|V
input gradient, at the width where the fused row-owner launches run."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sketchformer_amd import synthetic

pytestmark = pytest.mark.gpu

B, L = 16, 50
KW = dict(seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64)


def _engine(use_graph=False, **over):
    from sketchformer_amd import engine
    kw = dict(KW)
    kw.update(over)
    return engine.TrainEngine(engine.make_config(batch=B, dropout_rate=0.1, use_graph=use_graph, seed=9, **kw), init_seed=4)


@pytest.fixture(scope="module")
def batches():
    return [synthetic.token_batch(B, L, 1004, 345, seed=60 + i) for i in range(3)]


def _same_state(a, b):
    return torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v)


def _metric_bits(eng):
    return eng.metrics[:5].cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("over", [dict(), dict(class_buffer_layers=2), dict(attn_version=2), dict(do_classification=False),
                                  dict(do_reconstruction=False), dict(lowerdim=0, do_classification=False), dict(num_layers=1)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "default")
def test_moved_launches_are_ordered_in_every_model_structure(over, batches):
    """Which launches move differs with the structure: class buffers put two more Dense + dropout pairs on the side stream, without a
    class head only the metrics and the embedding gradient move, without a decoder nothing moves (no decoder-input event exists: the
    heads stay on the main stream), and one layer has no held group and no deferred input gradient - the main stream's only wait in
    front of the classifier backward is then the forward's wait for the K|V projection.  Two eager engines from one seed, 10 steps
    over 3 alternating batches: parameters and both Adam moments bit-equal, and finite."""
    a, b = _engine(**over), _engine(**over)
    for step in range(10):
        x, y = batches[step % 3]
        for e in (a, b):
            e.train_step(x, y)
    torch.cuda.synchronize()
    assert _same_state(a, b)
    for t in (a.params, a.adam_m, a.adam_v):
        assert np.isfinite(t.cpu().numpy()).all()


def test_step_metrics_equal_the_one_stream_step(batches):
    """A fresh eager engine (two streams: class head, class loss and metrics on the side stream) and a fresh use_graph = 1 engine (one
    stream, every launch where it always was) from the same seeds: their first forward runs on identical parameters with identical
    dropout masks and the same forward launch forms, so the five step metrics are bit-equal.  The parent commit, with every one of
    these launches on the main stream, gave bit equality here too (same box, same shapes): the move changes no value."""
    x, y = batches[0]
    got = []
    for use_graph in (False, True):
        eng = _engine(use_graph=use_graph)
        eng.train_step(x, y)
        torch.cuda.synchronize()
        got.append((_metric_bits(eng), eng.step_metrics()))
    print("eager      ", got[0][1])
    print("one stream ", got[1][1])
    assert all(np.isfinite(v) for v in got[0][1].values())
    assert np.array_equal(got[0][0], got[1][0]), (got[0][1], got[1][1])


def test_metrics_are_never_stale_and_never_overtaken(batches):
    """The metrics launch reads the four loss / hit sums on the side stream; the next step's loss launches overwrite them.  Engine A
    reads step_metrics() after every one of 8 steps (each read synchronises); engine B queues the same 8 steps without any host
    synchronisation and reads once.  The batches alternate, so consecutive steps have different losses: a read that ran before its
    step's sums were complete would repeat the previous step's figures (A), and a loss launch of step n + 1 that overtook the
    metrics launch of step n would change B's running state and, through nothing else, its last figures."""
    a, b = _engine(), _engine()
    seen = []
    for step in range(8):
        a.train_step(*batches[step % 3])
        seen.append(a.step_metrics())
    for step in range(8):
        b.train_step(*batches[step % 3])
    last_b = _metric_bits(b)
    torch.cuda.synchronize()
    assert np.array_equal(_metric_bits(a), last_b), (seen[-1], b.step_metrics())
    assert np.array_equal(a.metrics.cpu().numpy().view(np.uint32), b.metrics.cpu().numpy().view(np.uint32))      # running sums too
    assert _same_state(a, b)
    for prev, cur in zip(seen, seen[1:]):
        assert all(np.isfinite(v) for v in cur.values())
        assert cur["total_loss"] != prev["total_loss"] and cur["class_loss"] != prev["class_loss"] and cur["recon_loss"] != prev["recon_loss"], (prev, cur)


def test_call_kinds_interleaved_leave_no_stream_choice_behind(batches):
    """The class head runs on the side stream in a train step and on the main stream in every other call.  Engine A takes two train
    steps; engine B takes a train step, an inference forward, encode, a 4-step greedy decode, then the second train step: bit-equal
    parameters and moments - nothing of one call's stream choice (the deferred metrics launch, events, queues) reaches the next."""
    a, b = _engine(), _engine()
    b0, b1, b2 = batches
    a.train_step(*b0)
    a.train_step(*b1)
    b.train_step(*b0)
    b.forward(b2[0], training=False)
    b.encode(b1[0])
    b.greedy_decode(max_steps=4)
    b.train_step(*b1)
    torch.cuda.synchronize()
    assert _same_state(a, b)
    assert a.iterations == 2 and b.iterations == 2
    assert np.array_equal(_metric_bits(a), _metric_bits(b))


_CAPTURE = r"""
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from sketchformer_amd import engine, synthetic, _lib
B, L = 16, 50
kw = dict(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=2, vocab_size=1004, n_classes=345, lowerdim=64,
          dropout_rate=0.1, seed=9)
batches = [synthetic.token_batch(B, L, 1004, 345, seed=60 + i) for i in range(3)]
got = []
for mode, flag in ((0, 0), (2, _lib.MODEL_TWO_STREAM_GRAPH)):
    eng = engine.TrainEngine(engine.make_config(use_graph=mode, **kw), init_seed=4)
    eng.set_flags(flag)
    for step in range(5):
        eng.train_step(*batches[step %% 3])
    torch.cuda.synchronize()
    got.append((eng.params.clone(), eng.metrics[:5].cpu().numpy().view(np.uint32).copy()))
assert np.isfinite(got[0][0].cpu().numpy()).all()
assert torch.equal(got[0][0], got[1][0]), "parameters differ"
assert np.array_equal(got[0][1], got[1][1]), ("step metrics differ", got[0][1], got[1][1])
print("SIDE_MOVES_CAPTURE_OK")
"""


def test_two_stream_capture_keeps_the_moved_launches_bit_equal():
    """use_graph = 2 with MODEL_TWO_STREAM_GRAPH captures the same launches on the same two streams: the moved ones become nodes of the
    side branch, ordered by the same events.  Parameters and step metrics after 5 steps bit-equal to the eager engine's.  In a process
    of its own with a time limit: replaying a multi-branch graph has crashed inside the runtime in processes with many models behind
    them (test_two_stream_graph_capture_is_bit_equal_to_the_eager_step)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CAPTURE % root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SIDE_MOVES_CAPTURE_OK" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-800:])
