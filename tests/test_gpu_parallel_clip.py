"""Gradient clipping under data parallelism, on the two-rank scheme of tests/test_gpu_parallel.py (gloo on one device, RCCL when two
are visible): every rank computes the same global norm from the same all-reduced buffer (1/world_size enters as a factor on the
norm), so W ranks x B_local rows with a global threshold == one engine at batch W * B_local with the same threshold, within that
file's tolerance; the replicas stay identical and count the same iterations."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KW = dict(seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32,
          dropout_rate=0.0, use_graph=False, seed=5)
STEPS, B_LOCAL, START = 3, 4, 3000
CLIP = 0.05       # far below the gradient norm of this model at its initial weights (order 1): every step clips


def _batches(world):
    from sketchformer_amd import synthetic
    return [synthetic.token_batch(B_LOCAL * world, KW["seq_len"], KW["vocab_size"], KW["n_classes"], seed=70 + s) for s in range(STEPS)]


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
    eng = engine.TrainEngine(engine.make_config(batch=B_LOCAL, **dict(KW, use_graph=use_graph)), init_seed=1, process_group=pg)
    eng.dp_mode = dp_mode
    eng.set_gradient_clip(global_clipnorm=CLIP)
    eng.assert_replicas_equal()
    eng.state[0] = START
    scales = []
    for x, y in _batches(world):
        xs, ys = parallel.shard_batch(x, y, rank, world)
        eng.train_step(xs, ys)
        scales.append(eng.gradient_stats()["scale"])
    torch.cuda.synchronize()
    flat = eng.params.detach().cpu()
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat, group=pg)
    its = torch.tensor([eng.iterations], dtype=torch.int64)      # (host tensors, like `flat`)
    all_its = [torch.zeros_like(its) for _ in range(world)]
    dist.all_gather(all_its, its, group=pg)
    sc = torch.tensor(scales, dtype=torch.float64)
    all_sc = [torch.zeros_like(sc) for _ in range(world)]
    dist.all_gather(all_sc, sc, group=pg)
    if rank == 0:
        np.savez(out, flat=flat.numpy(), spread=float(max((g - flat).abs().max() for g in gathered)),
                 iters=np.array([int(t.item()) for t in all_its]), scales=np.stack([t.numpy() for t in all_sc]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,use_graph,dp_mode", [("gloo", False, "bucketed"), ("gloo", True, "bucketed"),
                                                       ("gloo", False, "single"), ("nccl", False, "bucketed")])
def test_two_clipped_ranks_equal_one_clipped_engine_at_double_batch(tmp_path, backend, use_graph, dp_mode):
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
    assert res["iters"].tolist() == [START + STEPS] * world                    # ... and count the same iterations
    assert np.array_equal(res["scales"][0], res["scales"][1])                  # the same norm on every rank, no extra collective
    ref = engine.TrainEngine(engine.make_config(batch=B_LOCAL * world, **KW), init_seed=1)
    ref.set_gradient_clip(global_clipnorm=CLIP)
    ref.state[0] = START
    ref_scales = []
    for x, y in _batches(world):
        ref.train_step(x, y)
        ref_scales.append(ref.gradient_stats()["scale"])
    torch.cuda.synchronize()
    assert ref.iterations == START + STEPS
    assert all(0.0 < s < 1.0 for s in ref_scales), ref_scales                  # the threshold was active on every step
    np.testing.assert_allclose(res["scales"][0], ref_scales, rtol=5e-3)      # (the tolerance of the parameters below)
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
    assert worst < 5e-3 * moved, (worst, moved)
