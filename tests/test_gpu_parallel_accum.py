"""Gradient accumulation under data parallelism, on the two-rank scheme of tests/test_gpu_parallel_clip.py (gloo on one device, RCCL
when two are visible): two ranks x B_local = 4 rows x k = 2 micro-batches == one engine at batch 16 within that file's tolerance (the
mean of equally sized shard gradients is the full-batch gradient, whether the shards are ranks or micro-batches); the replicas stay
identical and count the same iterations; and only the micro-step that closes an optimizer step reaches an all-reduce."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KW = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32,
          dropout_rate=0.0, use_graph=False, seed=5)
STEPS, B_LOCAL, K, START = 3, 4, 2, 3000


def _batches(world):
    from sketchformer_amd import synthetic
    return [synthetic.token_batch(B_LOCAL * world * K, KW["seq_len"], KW["vocab_size"], KW["n_classes"], seed=70 + s) for s in range(STEPS)]


def _worker(rank, world, port, out, backend, use_graph, dp_mode):
    local = rank if backend == "nccl" else 0
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(local), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)     # a wedged collective must not hold the GPU box
    import torch.distributed as dist
    from sketchformer_amd import engine, parallel
    torch.cuda.set_device(local)
    _, _, _, pg = parallel.init_from_env(backend=backend)
    calls = []                                            # every call of parallel.allreduce_*
    eng = engine.TrainEngine(engine.make_config(batch=B_LOCAL, **dict(KW, use_graph=use_graph)), init_seed=1, process_group=pg)
    for name in ("allreduce_flat_gradients", "allreduce_bucket"):
        def counted(*a, _fn=getattr(parallel, name), _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        setattr(parallel, name, counted)
    eng.dp_mode = dp_mode
    eng.set_gradient_accumulation(K)
    eng.assert_replicas_equal()
    eng.state[0] = START
    per_step = []
    for x, y in _batches(world):
        for j in range(K):                                # micro-batch j of the global batch, this rank's rows of it
            rows = slice(j * B_LOCAL * world, (j + 1) * B_LOCAL * world)
            xs, ys = parallel.shard_batch(x[rows], y[rows], rank, world)
            seen = len(calls)
            eng.train_step(xs, ys)
            per_step.append(len(calls) - seen)
    torch.cuda.synchronize()
    flat = eng.params.detach().cpu()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat, group=pg)
    its = torch.tensor([eng.iterations], dtype=torch.int64)      # (host tensors, like `flat`)
    all_its = [torch.zeros_like(its) for _ in range(world)]
    dist.all_gather(all_its, its, group=pg)
    if rank == 0:
        np.savez(out, flat=flat.numpy(), spread=float(max((g - flat).abs().max() for g in gathered)),
                 iters=np.array([int(t.item()) for t in all_its]), per_step=np.array(per_step), n_buckets=len(eng.grad_buckets()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,use_graph,dp_mode", [("gloo", False, "bucketed"), ("gloo", True, "bucketed"),
                                                       ("gloo", False, "single"), ("nccl", False, "bucketed")])
def test_two_accumulating_ranks_equal_one_engine_at_the_whole_batch(tmp_path, backend, use_graph, dp_mode):
    from sketchformer_amd import engine
    world = 2
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("the RCCL run needs >= 2 visible GPUs (one rank per device)")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "rank0.npz")
    mp.spawn(_worker, args=(world, port, out, backend, use_graph, dp_mode), nprocs=world, join=True)
    res = np.load(out)
    flat, spread = res["flat"], float(res["spread"])
    assert spread == 0.0                                                       # replicas stay identical ...
    assert res["iters"].tolist() == [START + STEPS] * world                    # ... and count optimizer steps, the same ones
    # only the closing micro-step communicates: one all-reduce per bucket (or one of the whole buffer) there, none on the others
    per_close = 1 if dp_mode == "single" else int(res["n_buckets"])
    assert res["per_step"].tolist() == ([0] * (K - 1) + [per_close]) * STEPS
    ref = engine.TrainEngine(engine.make_config(batch=B_LOCAL * world * K, **KW), init_seed=1)
    ref.state[0] = START
    for x, y in _batches(world):
        ref.train_step(x, y)
    torch.cuda.synchronize()
    assert ref.iterations == START + STEPS
    want = ref.params.detach().cpu().numpy()
    moved = np.abs(want - engine.keras_init(ref.entries, ref.n_floats, 1)).max()
    assert moved > 1e-3                                                        # the optimizer really moved the weights
    # (wk biases: analytically zero gradient, left out like in tests/test_gpu_parallel.py)
    worst = 0.0
    for e in ref.entries:
        if e["name"].endswith("wk/bias"):
            continue
        idx = (e["offset"] + np.arange(e["rows"])[:, None] * e["row_stride"] + np.arange(e["cols"])[None, :]).reshape(-1)
        worst = max(worst, float(np.abs(flat[idx] - want[idx]).max()))
    print("worst %.3e, moved %.3e, bound %.3e" % (worst, moved, 5e-3 * moved))
    assert worst < 5e-3 * moved, (worst, moved)
