#!/usr/bin/env python
"""Greedy reconstruction (predict_from_embedding) at the cfg-2 dimensions: B = 128 samples x 200 positions.
    python tools/decode_bench.py [--layerwise] [--attn-weights] [out.json]
  --layerwise     the layer-by-layer path of round 1 (skf_model_set_flags(SKF_MODEL_DECODE_LAYERWISE); the library reads no
                  environment)
  --attn-weights  also return the decoder's attention weights (skf_model_greedy_decode_attn; the host copy of the weights
                  is part of the timed call)"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketchformer_amd import engine
from sketchformer_amd import synthetic
from sketchformer_amd import _lib

layerwise = "--layerwise" in sys.argv
attn = "--attn-weights" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

B, L, V = 128, 200, 1004
cfg = engine.make_config(batch=B, seq_len=L, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=V, n_classes=345,
                         lowerdim=128, dropout_rate=0.0, use_graph=False, seed=1)
eng = engine.TrainEngine(cfg, init_seed=2)
x, _ = synthetic.token_batch(B, L, V, 345, seed=5)
eng.encode(x)
if layerwise:
    eng.set_flags(_lib.MODEL_DECODE_LAYERWISE)
sos, eos = V - 2, V - 1


def call():
    if attn:
        return eng.greedy_decode(None, sos=sos, eos=eos, with_attn_weights=True)[0]
    return eng.greedy_decode(None, sos=sos, eos=eos)


got = call()                                            # warm-up (graph capture / attribute calls)
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    got = call()
    ts.append(time.perf_counter() - t0)
t = float(np.median(ts))
npos = got.shape[1] - 1
t_dev = None
if attn:
    # the library call alone, into a preallocated device buffer: what the weight stores cost without the host copy
    import ctypes as C
    import torch
    aw = torch.empty(2 * cfg.num_layers, B, cfg.num_heads, L, L, dtype=torch.float32, device=eng.device)
    out = torch.empty(B, L + 1, dtype=torch.int64, device=eng.device)
    n_out = C.c_int(0)
    td = []
    for _ in range(6):
        t0 = time.perf_counter()
        _lib.call("skf_model_greedy_decode_attn", eng.handle, None, None, B, sos, eos, L, eng._p(out), C.byref(n_out), eng._p(aw),
                  eng._stream())
        eng.synchronize()
        td.append(time.perf_counter() - t0)
    t_dev = float(np.median(td[1:]))
rec = {"what": "greedy reconstruction, cfg-2 dimensions (4L/8H/d128/dff512, V=1004), B=128, random weights (no EOS: all %d positions)" % npos,
       "path": "layer-by-layer (51 launches / position)" if layerwise else "one launch / position",
       "attn_weights": attn, "seconds_all": ts, "seconds_per_call_device_only": t_dev,
       "positions": npos, "seconds_per_call": t, "ms_per_position": 1e3 * t / npos, "tokens_per_second": B * npos / t,
       "includes": "K/V projection of pre_decoder for all layers, host read-back of the result"}
print(json.dumps(rec))
if args:
    json.dump(rec, open(args[0], "w"), indent=1)
np.save("/tmp/decode_tokens_%s.npy" % ("unfused" if layerwise else "fused"), got)
