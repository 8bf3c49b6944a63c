"""Shared plumbing of the entry-point tests (test_gpu_continuous_ops, test_gpu_decode_step_ops, test_gpu_reduce_ops and the
LayerNorm / cast cases of test_gpu_ops and test_gpu_bf16_ops): pointer helpers, the comparison against a float64 reference and
the record of the worst error per entry point that profiles/entry_point_errors.txt is written from."""
import collections
import ctypes as C

import numpy as np
import torch

SENTINEL = -777.25                        # exactly representable in fp32 and bf16; no kernel under test produces it

WORST = collections.defaultdict(dict)     # entry point -> {quantity: worst error over the cases run so far}


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def ptr(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host64(t):
    return t.detach().float().cpu().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, np.float64)


def filled(*shape, dtype=torch.float32, value=SENTINEL):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def record(entry, quantity, err):
    WORST[entry][quantity] = max(WORST[entry].get(quantity, 0.0), float(err))


def close(got, want, rtol, entry, quantity, floor=1e-30):
    """max |got - want| <= rtol * max(max |want|, floor); the figure is recorded (report() prints the worst) before it is judged."""
    got, want = host64(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, (entry, quantity, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s %s: non-finite" % (entry, quantity)
    scale = max(float(np.abs(want).max()) if want.size else 0.0, floor)
    err = float(np.abs(got - want).max()) / scale if want.size else 0.0
    record(entry, quantity, err)
    assert err <= rtol, "%s %s: rel err %.3e > %.1e (scale %.3e)" % (entry, quantity, err, rtol, scale)


def report():
    """One line per entry point: the figures of profiles/entry_point_errors.txt."""
    print()
    for name in sorted(WORST):
        print("entry-point-error %-40s %s" % (name, "  ".join("%s %.2e" % kv for kv in sorted(WORST[name].items()))))
    WORST.clear()
