"""Weight averaging under data parallelism, on the two-rank scheme of tests/test_gpu_parallel_accum.py (gloo on one device): every
rank averages the same all-reduced parameters, so the shadows stay identical across ranks without a collective of their own - the
number of parallel.allreduce_* calls is that of the same steps without averaging - and the ranks count the same iterations."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KW = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32,
          dropout_rate=0.0, use_graph=False, seed=5)
STEPS, B_LOCAL, START, DECAY = 3, 4, 3000, 0.999


def _batches(world):
    from sketchformer_amd import synthetic
    return [synthetic.token_batch(B_LOCAL * world, KW["seq_len"], KW["vocab_size"], KW["n_classes"], seed=70 + s) for s in range(STEPS)]


def _worker(rank, world, port, out, dp_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import faulthandler
    faulthandler.dump_traceback_later(120, exit=True)     # a wedged collective must not hold the GPU box
    import torch.distributed as dist
    from sketchformer_amd import engine, parallel
    torch.cuda.set_device(0)
    _, _, _, pg = parallel.init_from_env(backend="gloo")
    calls = []                                            # every call of parallel.allreduce_*
    for name in ("allreduce_flat_gradients", "allreduce_bucket"):
        def counted(*a, _fn=getattr(parallel, name), _name=name, **kw):
            calls.append(_name)
            return _fn(*a, **kw)
        setattr(parallel, name, counted)
    counts, engines = {}, {}
    for averaging in (False, True):                       # the same steps without and with averaging
        eng = engine.TrainEngine(engine.make_config(batch=B_LOCAL, **KW), init_seed=1, process_group=pg)
        eng.dp_mode = dp_mode
        if averaging:
            eng.set_weight_average(DECAY, num_updates=True)
        eng.assert_replicas_equal()                       # (compares the shadow too)
        eng.state[0] = START
        seen = len(calls)
        for x, y in _batches(world):
            eng.train_step(*parallel.shard_batch(x, y, rank, world))
        torch.cuda.synchronize()
        counts[averaging], engines[averaging] = len(calls) - seen, eng
    eng, plain = engines[True], engines[False]
    eng.assert_replicas_equal()                           # still equal after the steps, shadow included
    same_training = bool(torch.equal(eng.params, plain.params) and torch.equal(eng.adam_m, plain.adam_m))
    shadow = eng.weight_average.detach().cpu()
    gathered = [torch.zeros_like(shadow) for _ in range(world)]
    dist.all_gather(gathered, shadow, group=pg)
    its = torch.tensor([eng.iterations], dtype=torch.int64)      # (host tensors, like `shadow`)
    all_its = [torch.zeros_like(its) for _ in range(world)]
    dist.all_gather(all_its, its, group=pg)
    if rank == 0:
        np.savez(out, identical=all(torch.equal(g.view(torch.int32), shadow.view(torch.int32)) for g in gathered),
                 lag=float((shadow - eng.params.cpu()).abs().max()), iters=np.array([int(t.item()) for t in all_its]),
                 calls_plain=counts[False], calls_avg=counts[True], n_buckets=len(eng.grad_buckets()), same_training=same_training)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("dp_mode", ["bucketed", "single"])
def test_two_averaging_ranks_keep_identical_shadows_without_an_extra_collective(tmp_path, dp_mode):
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "rank0.npz")
    mp.spawn(_worker, args=(world, port, out, dp_mode), nprocs=world, join=True)
    res = np.load(out)
    assert bool(res["identical"])                                              # the shadows are the same bits on every rank ...
    assert float(res["lag"]) > 0.0                                             # ... and really lag behind the weights
    assert res["iters"].tolist() == [START + STEPS] * world
    per_step = 1 if dp_mode == "single" else int(res["n_buckets"])
    assert int(res["calls_avg"]) == int(res["calls_plain"]) == per_step * STEPS      # no extra collective
    assert bool(res["same_training"])                                          # and the training itself is that of the plain engine
