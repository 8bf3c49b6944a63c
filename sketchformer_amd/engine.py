"""TrainEngine: owns the flat device buffers of one replica and drives the
C-ABI train step (skf_model_*).  Host-side mirror of what
``Transformer.build_model`` + ``prepare_model_trainer`` + ``train_on_batch`` set up
in the reference (models/sketchformer.py:63-129, 313-359).

Data parallelism (new functionality): one process per
GPU; every rank runs forward+backward on its shard of the global batch, the flat
fp32 gradient buffer is summed with ONE all-reduce (RCCL over xGMI on GPUs) and
the 1/world_size scale is fused into the Adam sweep.
"""
import ctypes as C
import os
import math

import numpy as np
import torch

from . import _lib
from ._lib import SkfConfig, SkfParamEntry

METRIC_NAMES = ("recon_loss", "recon_acc", "class_loss", "class_acc", "total_loss")


def positional_encoding(position, d_model):
    """builders/utils.py:12-32: float64 numpy angles with an np.float32(d_model)
    divisor, sin on even / cos on odd columns, cast to float32.  -> (position, d_model)."""
    pos = np.arange(position)[:, np.newaxis]
    i = np.arange(d_model)[np.newaxis, :]
    rates = 1 / np.power(10000, (2 * (i // 2)) / np.float32(d_model))
    ang = pos * rates
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return ang.astype(np.float32)


def make_config(batch, seq_len=200, d_model=128, num_heads=8, dff=512, num_layers=4, vocab_size=1004, n_classes=345,
                lowerdim=256, attn_version=1, continuous=False, blind_decoder_mask=True, dropout_rate=0.1,
                recon_weight=1.0, class_weight=1.0, lr_scheduler="WarmupDecay", lr=0.01, seed=0, use_graph=True,
                max_pos=1000, optimizer="Adam", class_buffer_layers=0, class_dropout=0.1, do_classification=True,
                do_reconstruction=True, gemm_precision=None, act_dtype="f32"):
    """gemm_precision: SKF_PREC_* arithmetic of the Dense / attention matmuls (0 fp32 MFMA, 6 bf16x6, 3 bf16x3);
    None = _lib.default_precision() (bf16x6 unless SKF_GEMM_PRECISION says otherwise).
    act_dtype: "f32" (the reference's arithmetic, cfg 1-4) or "bf16" (BASELINE cfg 5: bf16 activations / weight images /
    MFMA with fp32 accumulation, fp32 master weights and Adam)."""
    cfg = SkfConfig()
    cfg.act_dtype = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}[str(act_dtype).lower()]
    cfg.gemm_precision = _lib.default_precision() if gemm_precision is None else int(gemm_precision)
    cfg.batch, cfg.seq_len, cfg.d_model, cfg.num_heads, cfg.dff, cfg.num_layers = batch, seq_len, d_model, num_heads, dff, num_layers
    cfg.vocab_size, cfg.n_classes, cfg.lowerdim, cfg.attn_version = vocab_size or 0, n_classes, lowerdim, attn_version
    cfg.continuous, cfg.blind_decoder_mask, cfg.max_pos = int(continuous), int(blind_decoder_mask), max_pos
    cfg.dropout_rate, cfg.recon_weight, cfg.class_weight = dropout_rate, recon_weight, class_weight
    name = lr_scheduler.lower()
    if name in ("warmupdecay", "warmup-decay"):
        # models/sketchformer.py:113-114: warmup_steps=5000 hard-coded (hparams warmup_steps / lr ignored)
        cfg.schedule, cfg.sched_p0, cfg.sched_p1 = 0, float(d_model), float(5000 ** -1.5)
    elif name == "step-decay":
        # models/sketchformer.py:116-118 passes the non-existent kwarg min_lr= -> TypeError in the reference
        raise TypeError("__init__() got an unexpected keyword argument 'min_lr'")
    else:
        raise ValueError("unknown lr_scheduler %r" % lr_scheduler)
    cfg.beta1, cfg.beta2, cfg.eps = 0.9, 0.98, 1e-9   # models/sketchformer.py:122-124
    cfg.seed, cfg.use_graph = seed, int(use_graph)
    # models/sketchformer.py:120-126: Adam(schedule, 0.9, 0.98, 1e-9) or SGD(schedule, momentum=0.9)
    if optimizer.lower() == "adam":
        cfg.optimizer, cfg.momentum = 0, 0.0
    elif optimizer.lower() == "sgd":
        cfg.optimizer, cfg.momentum = 1, 0.9
    else:
        raise ValueError("unknown optimizer %r" % optimizer)
    cfg.class_buffer_layers, cfg.class_dropout = int(class_buffer_layers), float(class_dropout)
    cfg.do_classification, cfg.do_reconstruction = int(bool(do_classification)), int(bool(do_reconstruction))
    return cfg


def keras_init(entries, total, seed=0):
    """Keras default initialisers into a flat float32 numpy buffer
    (glorot_uniform Dense kernels, zeros biases, uniform(+-0.05) embeddings,
    ones/zeros LayerNorm, RandomNormal(0.05)/uniform(+-0.05) SelfAttnV1)."""
    rng = np.random.RandomState(seed)
    flat = np.zeros(total, dtype=np.float32)
    for e in entries:
        name = e["name"]
        r, c = e["rows"], e["cols"]
        view = strided_view(flat, e)
        if name.endswith("/kernel"):
            lim = math.sqrt(6.0 / (r + c))
            view[...] = rng.uniform(-lim, lim, size=(r, c))
        elif name.endswith("embedding") or name.endswith("V_attn"):
            view[...] = rng.uniform(-0.05, 0.05, size=(r, c))
        elif name.endswith("W_attn"):
            view[...] = rng.normal(0.0, 0.05, size=(r, c))
        elif name.endswith("/gamma"):
            view[...] = 1.0
    return flat


def strided_view(flat, e):
    """2-D numpy view of one variable inside a flat numpy buffer."""
    return np.lib.stride_tricks.as_strided(flat[e["offset"]:], shape=(e["rows"], e["cols"]),
                                           strides=(e["row_stride"] * flat.itemsize, flat.itemsize))


def param_entries(cfg):
    lib = _lib.load()
    n = lib.skf_model_param_entries(C.byref(cfg), None, 0)
    if n < 0:
        _lib.check(n, "skf_model_param_entries")
    arr = (SkfParamEntry * n)()
    lib.skf_model_param_entries(C.byref(cfg), arr, n)
    return [{"name": a.name.decode(), "offset": int(a.offset), "rows": int(a.rows), "cols": int(a.cols),
             "row_stride": int(a.row_stride)} for a in arr]


# shapes as the reference's trainable variables report them (1-D variables, (U,1) V_attn, (1,L) expand kernel)
def logical_shape(e):
    n = e["name"]
    if n.endswith(("/bias", "/gamma", "/beta", "b_attn")):
        return (e["cols"],)
    return (e["rows"], e["cols"])


SAMPLING_NEEDS_TOKENS = ("sampled decoding is built for token models: a continuous model has a regression head and three pen "
                         "logits, no categorical distribution over tokens to draw from")


SCORING_NEEDS_TOKENS = ("teacher-forced scoring is built for token models: a continuous model has a regression head and three pen "
                        "logits, no categorical distribution that gives a token sequence a likelihood")


def check_sampling(temperature, top_k, top_p):
    """The parameter ranges of the selection rule (include/skf.h: SkfSampling); ValueError outside them."""
    if not float(temperature) > 0.0 or float(temperature) == float("inf"):
        raise ValueError("temperature must be a finite number > 0 (got %r)" % (temperature,))
    if int(top_k) != top_k or int(top_k) < 0:
        raise ValueError("top_k must be an integer >= 0, 0 = off (got %r)" % (top_k,))
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError("top_p must be in (0, 1], 1 = off (got %r)" % (top_p,))


BEAM_NEEDS_TOKENS = ("beam search is built for token models: a continuous model decodes one deterministic stroke-5 row per "
                     "position, with nothing to rank")


def check_beam(beam_width, length_alpha, vocab_size=None, batch=None):
    """The parameter ranges of beam search (include/skf.h: SkfBeam); ValueError outside them."""
    if int(beam_width) != beam_width or not 1 <= int(beam_width) <= _lib.BEAM_MAX:
        raise ValueError("beam_width must be an integer in [1, %d] (got %r)" % (_lib.BEAM_MAX, beam_width))
    for what, cap in (("vocab_size", vocab_size), ("batch", batch)):
        if cap is not None and int(beam_width) > cap:
            raise ValueError("beam_width must not exceed %s=%d (got %r)" % (what, cap, beam_width))
    if not float(length_alpha) >= 0.0 or float(length_alpha) == float("inf"):
        raise ValueError("length_alpha must be a finite number >= 0 (got %r)" % (length_alpha,))


def check_gradient_clip(clipnorm=None, global_clipnorm=None, clipvalue=None):
    """The rule of the clip settings (tf.keras optimizers': at most one of the three; include/skf.h: skf_gradient_clip_validate),
    free of the device.  None or 0 = not set.  -> (mode, threshold, clipvalue) as the C entries take them: mode 0 none, 1 per
    variable (clipnorm), 2 global (global_clipnorm).  ValueError for two settings at once and for a value that is not a finite
    number > 0."""
    given = {k: float(v) for k, v in (("clipnorm", clipnorm), ("global_clipnorm", global_clipnorm), ("clipvalue", clipvalue))
             if v is not None and v != 0}
    if len(given) > 1:
        raise ValueError("at most one of clipnorm, global_clipnorm and clipvalue may be set (got %s)" % ", ".join(sorted(given)))
    for k, v in given.items():
        if not 1e-38 <= v <= 3.4028234663852886e38:      # (a normal float32: the library takes it as one)
            raise ValueError("%s must be a finite number > 0 (got %r)" % (k, v))
    if "clipnorm" in given:
        return 1, given["clipnorm"], 0.0
    if "global_clipnorm" in given:
        return 2, given["global_clipnorm"], 0.0
    return 0, 0.0, given.get("clipvalue", 0.0)


# The most micro-batches one optimizer step may sum.  The sum is carried in fp32: its rounding error grows like k * 2^-24 relative to
# the largest partial sum, 2^-14 (6e-5) at 1024 - still an order of magnitude below the 2^-9 of the bf16 activations the cfg-5
# gradients are computed from - and 1 / (world_size * k) stays far inside the normal float32 range.  Beyond it a value is far more
# likely a slip (a batch size in the wrong field) than a plan.
ACCUM_STEPS_MAX = 1024


def check_gradient_accumulation(steps):
    """The rule of ``accum_steps`` (host only): an integer in [1, ACCUM_STEPS_MAX]; 1 = no accumulation.  bool and float are refused
    (True is not a count, and 2.0 usually is the result of a division that may as well give 2.5).  -> int; ValueError otherwise."""
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)):
        raise ValueError("accum_steps must be an integer (got %r of type %s)" % (steps, type(steps).__name__))
    if not 1 <= int(steps) <= ACCUM_STEPS_MAX:
        raise ValueError("accum_steps must be in [1, %d] (got %r)" % (ACCUM_STEPS_MAX, steps))
    return int(steps)


def check_weight_average(decay):
    """The rule of a weight-average ``decay`` (host only; skf_weight_average_validate): a finite number strictly between 0 and 1 -
    0 would make the average the weights themselves, 1 would freeze it.  bool is refused.  -> float; ValueError otherwise."""
    if isinstance(decay, (bool, np.bool_)) or not isinstance(decay, (int, float, np.integer, np.floating)):
        raise ValueError("the decay of a weight average must be a number (got %r of type %s)" % (decay, type(decay).__name__))
    d = float(np.float32(decay))
    if _lib.load().skf_weight_average_validate(d) != 0:
        raise ValueError("the decay of a weight average must be finite and lie in (0, 1) as a float32 (got %r)" % (decay,))
    return d


COMPLETION_NEEDS_TOKENS = ("sketch completion is built for token models: a prefix is a sequence of tokens, and continuous (stroke-5) "
                           "prefixes are not built")


def check_prefix(prefix, prefix_len, rows, max_steps, vocab_size, eos=0):
    """The prefix of a completion (include/skf.h: prefix-forced decoding) as the C entries take it: ``(tokens, lens)`` with tokens a
    (rows, ld) int64 array - or device tensor when ``prefix`` is one - and lens (rows,) int32, 0 <= lens <= max_steps, ld >= 1.
    prefix: at most ``rows`` rows of at least max(len) tokens; prefix_len: one length per given row, or None = each row's tokens up to
    (not including) its first ``eos`` or PAD (0).  Rows beyond the given ones take row 0's prefix and length, so that a short batch
    does not pull the shortest prefix - where the position loop starts - down to 0.  ValueError for a length outside [0, max_steps]
    or beyond the prefix's columns, and for a host-side prefix with a token outside [0, vocab_size) among the forced ones (a device
    tensor is trusted, like every device input; the kernels treat such a token as PAD)."""
    on_device = torch.is_tensor(prefix) and prefix.is_cuda
    host = prefix.detach().cpu().numpy() if torch.is_tensor(prefix) else np.asarray(prefix)
    if host.ndim != 2 or not 1 <= host.shape[0] <= rows:
        raise ValueError("prefix must be a 2-D array of 1 .. %d rows (got shape %r)" % (rows, tuple(host.shape)))
    if not np.issubdtype(host.dtype, np.integer):
        raise ValueError("prefix must hold integer tokens (got dtype %s)" % host.dtype)
    host = host.astype(np.int64)
    n, width = host.shape
    if prefix_len is None:
        stop = (host == int(eos)) | (host == 0)
        lens = np.where(stop.any(axis=1), stop.argmax(axis=1), width).astype(np.int64)
    else:
        lens = np.asarray(prefix_len).astype(np.int64).reshape(-1)
        if len(lens) != n:
            raise ValueError("prefix_len must give one length per prefix row (%d rows, %d lengths)" % (n, len(lens)))
    if (lens < 0).any() or (lens > max_steps).any():
        raise ValueError("a prefix length must be in [0, max_steps = %d] (got %d .. %d)" % (max_steps, lens.min(), lens.max()))
    if (lens > width).any():
        raise ValueError("a prefix length exceeds the prefix's %d columns (got %d)" % (width, lens.max()))
    forced = np.arange(width)[None, :] < lens[:, None]
    if not on_device and forced.any():
        lo, hi = int(host[forced].min()), int(host[forced].max())
        if lo < 0 or hi >= vocab_size:
            raise ValueError("prefix token out of range: values span [%d, %d], valid range is [0, %d)" % (lo, hi, vocab_size))
    ld = max(width, 1)
    all_lens = np.full(rows, lens[0], dtype=np.int32)
    all_lens[:n] = lens
    if on_device:
        tokens = prefix.new_zeros((rows, ld), dtype=torch.int64)
        tokens[:n, :width] = prefix
        tokens[n:, :width] = prefix[0]
    else:
        tokens = np.zeros((rows, ld), dtype=np.int64)
        tokens[:n, :width] = host
        tokens[n:, :width] = host[0]
    return tokens, all_lens


class TrainEngine:
    """One replica of the sketch-transformer-tf2 train step on one GPU."""

    def __init__(self, cfg, device=None, init_seed=0, process_group=None):
        if not torch.cuda.is_available():
            raise _lib.SkfError("TrainEngine needs a HIP device: torch.cuda.is_available() is False (no CPU fallback)")
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        _lib.call("skf_config_validate", C.byref(cfg))
        self.entries = param_entries(cfg)
        self.by_name = {e["name"]: e for e in self.entries}
        self.n_floats = int(self.lib.skf_model_param_floats(C.byref(cfg)))
        flat = keras_init(self.entries, self.n_floats, init_seed)
        dev = self.device
        self._params = torch.from_numpy(flat).to(dev)
        self._grads = torch.zeros(self.n_floats, dtype=torch.float32, device=dev)
        self._adam_m = torch.zeros_like(self._grads)
        self._adam_v = torch.zeros_like(self._grads)
        self.pos = torch.from_numpy(positional_encoding(cfg.max_pos, cfg.d_model)).to(dev)
        self._metrics = torch.zeros(32, dtype=torch.float32, device=dev)
        self._state = torch.zeros(int(self.lib.skf_step_state_bytes()) // 8 + 1, dtype=torch.int64, device=dev)
        ws_bytes = int(self.lib.skf_model_workspace_bytes(C.byref(cfg)))
        self._workspace = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        off = (-self._workspace.data_ptr()) % 256
        self._ws_ptr = self._workspace.data_ptr() + off
        self._ws_bytes = ws_bytes
        handle = C.c_void_p()
        _lib.call("skf_model_create", C.byref(cfg), C.byref(handle))
        self.handle = handle
        _lib.call("skf_model_bind", handle, self._p(self._params), self._p(self._grads), self._p(self._adam_m),
                  self._p(self._adam_v), self._p(self.pos), C.c_void_p(self._ws_ptr), ws_bytes, self._p(self._metrics),
                  self._p(self._state))
        # a dedicated non-default stream: hipGraph capture is illegal on the legacy default stream
        self.stream = torch.cuda.Stream(device=dev)
        self._depth = 0
        self._dirty = False
        # A/B knob of the Python layer, read once: "1" = a train step clones the caller's device inputs like round 5 (see _stage)
        self._step_clones = os.environ.get("SKF_CLONE_INPUTS") == "1"
        self._comm = None                # communication stream of the data-parallel gradient buckets
        self.pg = process_group
        self.world_size = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.rank = torch.distributed.get_rank(process_group) if process_group is not None else 0
        # "bucketed": the flat gradient buffer is all-reduced in the pieces backward finishes (overlapping the rest of
        # backward / the optimizer sweep of the previous piece); "single": ONE all-reduce of the whole buffer after
        # backward (the literal north-star schedule) - bench.py --allreduce single|bucketed A/Bs the two
        self.dp_mode = "bucketed"
        self._clip = None                # set_gradient_clip: the settings, the clip workspace and its stats words
        self._accum = None               # set_gradient_accumulation: {"k", "acc", "pending"}
        self._avg = None                 # set_weight_average: {"decay", "num_updates", "shadow", "live"}

    # The buffers live on the engine's stream.  A step no longer makes the caller's stream wait for it (that hand-over, and the
    # one back at the start of the next step, were two cross-stream hops = ~25-40 us of idle GPU between steps,
    # profiles/r03l_gaps.txt): it only marks the results unpublished, and whoever READS a buffer through the attributes below
    # (or any accessor of this class) first orders the current stream behind the engine's.
    def _publish(self):
        if self._dirty:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            self._dirty = False

    def _published(self, t):
        self._publish()
        return t

    params = property(lambda self: self._published(self._params))
    grads = property(lambda self: self._published(self._grads))
    adam_m = property(lambda self: self._published(self._adam_m))
    adam_v = property(lambda self: self._published(self._adam_v))
    metrics = property(lambda self: self._published(self._metrics))
    state = property(lambda self: self._published(self._state))
    workspace = property(lambda self: self._published(self._workspace))
    # the averaged weights (set_weight_average), None without averaging; while ``average_live`` it holds the raw weights instead
    weight_average = property(lambda self: None if self._avg is None else self._published(self._avg["shadow"]))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                self.lib.skf_model_destroy(h)
            except Exception:
                pass

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _stream(self):
        return C.c_void_p(self.stream.cuda_stream)

    def _enter(self):
        # order after whatever the caller queued on its current stream (H2D copies of the batch, set()).  Nested calls (train_step
        # brackets forward_backward + apply_gradients) hand over once: every hand-over is a cross-stream event pair, and the one
        # that used to sit between the backward and the optimizer was ~40 us of idle GPU per step (profiles/r03l_gaps.txt)
        if self._depth == 0:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self._depth += 1

    def _leave(self):
        # let the caller's stream observe the step's results
        self._depth -= 1
        if self._depth == 0:
            self._dirty = True               # published lazily (see _publish)

    def synchronize(self):
        self.stream.synchronize()

    # ---- parameters by (Keras-style) name
    def _view(self, flat, name):
        e = self.by_name[name]
        return torch.as_strided(flat, (e["rows"], e["cols"]), (e["row_stride"], 1), e["offset"])

    def get(self, name, which="params"):
        e = self.by_name[name]
        return self._view(getattr(self, which), name).detach().cpu().numpy().reshape(logical_shape(e)).copy()

    def set(self, name, value, which="params"):
        v = self._view(getattr(self, which), name)
        v.copy_(torch.as_tensor(np.asarray(value, dtype=np.float32).reshape(v.shape)).to(self.device))

    def state_dict_numpy(self, which="params"):
        return {e["name"]: self.get(e["name"], which) for e in self.entries}

    def load_numpy(self, params, which="params"):
        for k, v in params.items():
            self.set(k, v, which)

    # ---- steps
    def _dev_tokens(self, x, clone, limit=None, what="token id"):
        """int64 device copy (``clone``: see _own).  Host inputs (the loader's numpy batches) are range-checked against ``limit`` here - a
        tokenizer / vocab_size (or class count) mismatch must fail loudly instead of training on wrong rows; tensors
        that already live on the device are trusted (checking them would cost a host sync per step)."""
        t = torch.as_tensor(x)
        if limit is not None and not t.is_cuda and t.numel():
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= limit:
                raise ValueError("%s out of range: values span [%d, %d], valid range is [0, %d) - tokenizer / dataset "
                                 "does not match the model (vocab_size / n_classes)" % (what, lo, hi, limit))
        if t.dtype != torch.int64:
            t = t.to(torch.int64)
        return self._own(t, t.to(self.device, non_blocking=True).contiguous(), clone)

    def _own(self, given, staged, clone):
        """The step reads its inputs asynchronously on the engine's stream and no longer makes the caller's stream wait for it
        (_publish): a device tensor the caller passes in - and may refill IN PLACE for the next batch - is therefore copied here,
        on the caller's stream (the hand-over of _enter orders the step behind the copy).  Host inputs already became fresh device
        copies.  ~2 us of copy kernels on the caller's stream, nothing on the engine's.  ``clone=False`` is for _stage alone: there the
        caller's stream waits for the library's staging copy instead."""
        if clone and torch.is_tensor(given) and given.is_cuda and staged.data_ptr() == given.data_ptr():
            return staged.clone()
        return staged

    def _dev_input(self, x, clone):
        """(B,L) int64 tokens, or (B,L,5) float32 stroke-5 rows in continuous mode (the reference casts the
        loader's float64 to float32 at the tf.function boundary, models/sketchformer.py:317-319)."""
        if not self.cfg.continuous:
            return self._dev_tokens(x, clone, self.cfg.vocab_size)
        t = torch.as_tensor(x)
        if t.dim() != 3 or t.shape[-1] != 5:
            raise ValueError("continuous mode expects (B, L, 5) stroke-5 input")
        return self._own(t, t.to(self.device, dtype=torch.float32, non_blocking=True).contiguous(), clone)

    def _hold(self, *tensors):
        """The engine's stream reads these caller-owned tensors asynchronously: tell the caching allocator, so that a tensor the
        caller drops right after the call is not handed out again (and overwritten from the caller's stream) before the step has
        staged it (the step used to make the caller's stream wait instead: see _publish)."""
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(self.stream)

    def _ld(self, t):
        return t.stride(0) // 5 if self.cfg.continuous else t.stride(0)

    def forward(self, inp, tar=None, training=False):
        """Transformer.call: fills the internal buffers (see ``buffer``)."""
        inp = self._dev_input(inp, clone=True)
        tar = inp if tar is None else self._dev_input(tar, clone=True)
        self._enter()
        try:
            self._hold(inp, tar)
            _lib.call("skf_model_forward", self.handle, self._p(inp), self._p(tar), self._ld(tar), int(training), self._stream())
        finally:
            self._leave()

    def set_flags(self, flags):
        """skf_model_set_flags: per-model switches (``_lib.MODEL_DECODE_LAYERWISE``)."""
        _lib.check(self.lib.skf_model_set_flags(self.handle, int(flags)), "skf_model_set_flags")

    def encode(self, inp):
        """encode_from_seq (models/sketchformer.py:162-168): encoder + bottleneck + classifier, dropout off.
        Results in the buffers 'embedding', 'class_probs', 'enc_output'."""
        inp = self._dev_input(inp, clone=True)
        self._enter()
        try:
            self._hold(inp)
            _lib.call("skf_model_encode", self.handle, self._p(inp), self._stream())
        finally:
            self._leave()

    def _prefix(self, prefix, prefix_len, prefill, rows, max_steps, eos):
        """check_prefix, then the prefix on the device and the SkfPrefix that points at it -> (SkfPrefix, what must stay alive)."""
        if self.cfg.continuous:
            raise ValueError(COMPLETION_NEEDS_TOKENS)
        tokens, lens = check_prefix(prefix, prefix_len, rows, max_steps, self.cfg.vocab_size, eos)
        dev = torch.as_tensor(tokens).to(self.device).contiguous()
        arr = (C.c_int * rows)(*lens.tolist())
        pf = _lib.SkfPrefix(tokens=dev.data_ptr(), ld=int(dev.shape[1]), len_host=arr, stepwise=0 if prefill else 1)
        return pf, (dev, arr)

    def greedy_decode(self, embedding=None, expected_len=None, n_valid=None, sos=0, eos=0, max_steps=None,
                      with_attn_weights=False, prefix=None, prefix_len=None, prefill=True):
        """predict_from_embedding (models/sketchformer.py:255-311) with a K/V cache.  embedding: (B,d) array / tensor
        or None (= the model's own 'embedding' buffer, i.e. right after ``encode``).  Returns the reconstruction as a
        host array: (n_valid, T) int32 tokens incl. the SOS column, or (n_valid, T, 5) float32 stroke-5 rows.
        with_attn_weights: return ``(recon, weights)`` instead, weights = the reference's res['attn_weights']
        (builders/layers/transformer.py:328-344): {'decoder_layer{i}_block1': (n_valid, H, T-1, T-1),
        'decoder_layer{i}_block2': (n_valid, H, T-1, seq_len)} float32, the last decoder pass over recon[:, :T-1]
        (skf_model_greedy_decode_attn).  A non-blind decoder needs expected_len for it (ValueError otherwise).
        prefix, prefix_len: sketch completion (skf_model_prefix_decode; the rule is in include/skf.h, the arguments in
        ``check_prefix``): the first prefix_len[b] tokens of row b are given and the decoder goes on from there; the result holds
        them in columns 1 .. prefix_len[b].  prefill=True produces the cache rows of the given positions in num_layers launches
        before the position loop, False steps through them one launch each; the results are the same bits.  Token models only,
        and not together with with_attn_weights (ValueError)."""
        B, L = self.cfg.batch, self.cfg.seq_len
        n_valid = B if n_valid is None else int(n_valid)
        max_steps = L if max_steps is None else int(max_steps)
        if prefix is not None:
            if with_attn_weights:
                raise ValueError("the attention weights of a completion are not built: with_attn_weights and prefix exclude each other")
            pf, keep = self._prefix(prefix, prefix_len, prefill, B, max_steps, eos)
            return self._decode_call("skf_model_prefix_decode", embedding, expected_len, n_valid, sos, eos, max_steps, C.byref(pf),
                                     None, None)[0]
        if with_attn_weights and not self.cfg.blind_decoder_mask and expected_len is None:
            raise ValueError("attention weights of a non-blind decoder need expected_len: with nattn = i + 1 the rows decoded "
                             "earlier were masked differently from the reference's last pass")
        aw = None
        if with_attn_weights:       # every row of a decoded position is written by the kernels: no memset
            aw = torch.empty(2 * self.cfg.num_layers, B, self.cfg.num_heads, max_steps, L, dtype=torch.float32,
                             device=self.device)
        if aw is None:
            return self._decode_call("skf_model_greedy_decode", embedding, expected_len, n_valid, sos, eos, max_steps)[0]
        res, n_out = self._decode_call("skf_model_greedy_decode_attn", embedding, expected_len, n_valid, sos, eos, max_steps, self._p(aw))
        T = n_out - 1
        weights = {}
        for i in range(self.cfg.num_layers):
            weights['decoder_layer%d_block1' % (i + 1)] = aw[2 * i, :n_valid, :, :T, :T].cpu().numpy()
            weights['decoder_layer%d_block2' % (i + 1)] = aw[2 * i + 1, :n_valid, :, :T, :].cpu().numpy()
        return res, weights

    def sample_decode(self, embedding=None, expected_len=None, n_valid=None, sos=0, eos=0, max_steps=None,
                      temperature=1.0, top_k=0, top_p=1.0, seed=0, stream_ids=None, prefix=None, prefix_len=None, prefill=True):
        """greedy_decode with every token drawn instead of maximised (skf_model_sample_decode; the selection rule is in
        include/skf.h): logits / temperature, then the top_k largest (0 = off; ties at the threshold all stay), then the nucleus
        of mass top_p (1 = off), then an inverse-CDF draw in index order with u = skf_sample_uniform(seed, stream_ids[b], position).
        stream_ids: one integer per batch row (default 0 .. B-1); a row's draws depend on its stream id, not on its batch slot.
        Token models only (ValueError for a continuous one).  Returns (n_valid, T) int32 incl. the SOS column, like greedy_decode.
        prefix, prefix_len, prefill: as in greedy_decode; a position keeps its uniform whether or not positions before it were given."""
        B, L = self.cfg.batch, self.cfg.seq_len
        if self.cfg.continuous:
            raise ValueError(SAMPLING_NEEDS_TOKENS)
        check_sampling(temperature, top_k, top_p)
        n_valid = B if n_valid is None else int(n_valid)
        max_steps = L if max_steps is None else int(max_steps)
        sid = None
        if stream_ids is not None:
            v = np.asarray(stream_ids).astype(np.int64).reshape(-1)
            if len(v) > B or (v < 0).any() or (v >= 2 ** 31).any():
                raise ValueError("stream_ids: at most batch=%d integers in [0, 2^31)" % B)
            arr = np.arange(B, dtype=np.int64)
            arr[:len(v)] = v
            sid = (C.c_int * B)(*arr.tolist())
        smp = _lib.SkfSampling(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed) & 0xffffffff)
        if prefix is not None:
            pf, keep = self._prefix(prefix, prefix_len, prefill, B, max_steps, eos)
            return self._decode_call("skf_model_prefix_decode", embedding, expected_len, n_valid, sos, eos, max_steps, C.byref(pf),
                                     C.byref(smp), sid)[0]
        return self._decode_call("skf_model_sample_decode", embedding, expected_len, n_valid, sos, eos, max_steps, C.byref(smp), sid)[0]

    def beam_decode(self, embedding, expected_len=None, n_valid=None, sos=0, eos=0, max_steps=None, beam_width=4,
                    length_alpha=0.0):
        """Beam-search reconstruction (skf_model_beam_decode; the selection rule is in include/skf.h): the beam_width most likely
        reconstructions of n = batch // beam_width sketches.  embedding: (n, E) array / tensor [(n, L, d) without a bottleneck];
        expected_len: one length per sketch, required by a non-blind decoder.  Returns (tokens (n_valid, W, T) int32 incl. the SOS
        column, scores (n_valid, W) float32: the sums of log p, lengths (n_valid, W) int32: the position of a hypothesis's EOS, or
        the positions decoded when it has none); the hypotheses of a sketch are ordered by score / ((5 + length) / 6)^length_alpha,
        best first.  Token models only (ValueError for a continuous one).  ``beam_complete`` is the same search behind a prefix."""
        return self._beam_search(embedding, expected_len, n_valid, sos, eos, max_steps, beam_width, length_alpha, None, None)

    def beam_complete(self, embedding, prefix, prefix_len=None, expected_len=None, n_valid=None, sos=0, eos=0, max_steps=None,
                      beam_width=4, length_alpha=0.0):
        """beam_decode behind a prefix (skf_model_beam_prefix_decode; the rule is in include/skf.h): one prefix per sketch, given like
        greedy_decode's (``check_prefix``); every hypothesis starts with its sketch's prefix and the scores are
        log p(continuation | prefix, embedding).  Beams always step through the prefix: there is no prefill under an ancestry table.
        Same returns as beam_decode."""
        if prefix is None:
            raise ValueError("beam_complete needs a prefix; beam_decode searches from the start symbol")
        return self._beam_search(embedding, expected_len, n_valid, sos, eos, max_steps, beam_width, length_alpha, prefix, prefix_len)

    def _beam_search(self, embedding, expected_len, n_valid, sos, eos, max_steps, beam_width, length_alpha, prefix, prefix_len):
        """beam_decode (prefix None) and beam_complete: checks, buffers, the C entry, the host copies"""
        B, L = self.cfg.batch, self.cfg.seq_len
        if self.cfg.continuous:
            raise ValueError(BEAM_NEEDS_TOKENS)
        check_beam(beam_width, length_alpha, self.cfg.vocab_size, B)
        W = int(beam_width)
        n = B // W
        if not self.cfg.blind_decoder_mask and expected_len is None:
            raise ValueError("beam search of a non-blind decoder needs expected_len")
        n_valid = n if n_valid is None else int(n_valid)
        if not 1 <= n_valid <= n:
            raise ValueError("n_valid must be in [1, batch // beam_width = %d]" % n)
        max_steps = L if max_steps is None else int(max_steps)
        e = self._decode_embedding(embedding, rows=n)
        lim = self._expected_len(expected_len, rows=n)
        out = torch.zeros(n, W, max_steps + 1, dtype=torch.int64, device=self.device)
        scores = torch.zeros(n, W, dtype=torch.float32, device=self.device)
        lengths = torch.zeros(n, W, dtype=torch.int32, device=self.device)
        n_out = C.c_int(0)
        bm = _lib.SkfBeam(beam_width=W, length_alpha=float(length_alpha))
        pf = None
        if prefix is not None:
            pf, keep = self._prefix(prefix, prefix_len, False, n, max_steps, eos)
        self._enter()
        try:
            if pf is not None:
                _lib.call("skf_model_beam_prefix_decode", self.handle, self._p(e), lim, n_valid, int(sos), int(eos), max_steps,
                          self._p(out), self._p(scores), self._p(lengths), C.byref(n_out), C.byref(bm), C.byref(pf), self._stream())
            else:
                _lib.call("skf_model_beam_decode", self.handle, self._p(e), lim, n_valid, int(sos), int(eos), max_steps, self._p(out),
                          self._p(scores), self._p(lengths), C.byref(n_out), C.byref(bm), self._stream())
        finally:
            self._leave()
        self.synchronize()
        return (out[:n_valid, :, :n_out.value].cpu().numpy().astype(np.int32), scores[:n_valid].cpu().numpy(),
                lengths[:n_valid].cpu().numpy())

    def score(self, inp, tar=None, n_valid=None, eos=0):
        """Teacher-forced scoring (skf_sequence_score; the rule is in include/skf.h): ``forward(inp, tar, training=False)``, then the
        log-likelihood and the rank of every token tar[:, 1:seq_len] under the 'logits' buffer, fp32 or bf16 model alike.  tar=None
        scores the input against itself (the autoencoding objective).  A sequence is scored through its first ``eos`` (to its first
        PAD without one).  The scoring launches follow the forward on the engine's stream and the caller's stream is ordered behind
        them; there is no host synchronisation.  Returns device tensors for the first n_valid rows: (tok_logp (n, seq_len - 1)
        float32, tok_rank (n, seq_len - 1) int32, seq_logp (n,) float32, seq_len (n,) int32).  Token models with a reconstruction
        head only (ValueError otherwise)."""
        if self.cfg.continuous:
            raise ValueError(SCORING_NEEDS_TOKENS)
        if not self.cfg.do_reconstruction:
            raise ValueError("do_reconstruction is off: the model has no decoder whose logits could be scored")
        B, L, V = self.cfg.batch, self.cfg.seq_len, self.cfg.vocab_size
        T = L - 1
        n_valid = B if n_valid is None else int(n_valid)
        if not 1 <= n_valid <= B:
            raise ValueError("n_valid must be in [1, batch = %d]" % B)
        inp = self._dev_input(inp, clone=True)
        tar = inp if tar is None else self._dev_input(tar, clone=True)
        if tar.dim() != 2 or tar.shape[0] != B or tar.shape[1] < L:
            raise ValueError("tar must hold batch=%d rows of at least seq_len=%d tokens (got %r)" % (B, L, tuple(tar.shape)))
        # allocated on the caller's stream BEFORE the hand-over; written on the engine's
        tok_logp = torch.empty(B, T, dtype=torch.float32, device=self.device)
        tok_rank = torch.empty(B, T, dtype=torch.int32, device=self.device)
        seq_logp = torch.empty(B, dtype=torch.float32, device=self.device)
        seq_len = torch.empty(B, dtype=torch.int32, device=self.device)
        self._enter()
        try:
            self._hold(inp, tar, tok_logp, tok_rank, seq_logp, seq_len)
            _lib.call("skf_model_forward", self.handle, self._p(inp), self._p(tar), self._ld(tar), 0, self._stream())
            ptr, rows, cols, ld, is16 = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
            _lib.call("skf_model_buffer_info", self.handle, b"logits", C.byref(ptr), C.byref(rows), C.byref(cols), C.byref(ld),
                      C.byref(is16))
            if rows.value != B * T or cols.value != V:
                raise _lib.SkfError("the 'logits' buffer is (%d, %d), expected (%d, %d)" % (rows.value, cols.value, B * T, V))
            _lib.call("skf_sequence_score", ptr, is16.value, ld.value, B, T, V, self._p(tar), tar.stride(0), 1, int(eos),
                      self._p(tok_logp), self._p(tok_rank), self._p(seq_logp), self._p(seq_len), self._stream())
        finally:
            self._leave()
        self._publish()          # the caller's stream waits for the engine's (an event, not the host)
        return tok_logp[:n_valid], tok_rank[:n_valid], seq_logp[:n_valid], seq_len[:n_valid]

    def _decode_embedding(self, embedding, rows=None):
        """The caller's embedding as a float32 device tensor of the shape the decoder starts from (``rows`` of them: the batch
        unless given), or None for None."""
        if embedding is None:
            return None
        B, L = self.cfg.batch if rows is None else rows, self.cfg.seq_len
        e = torch.as_tensor(np.asarray(embedding, dtype=np.float32) if not torch.is_tensor(embedding) else embedding)
        e = e.to(self.device, dtype=torch.float32).contiguous()
        if self.cfg.lowerdim == 0:      # no bottleneck: the "embedding" is the encoder output (B, L, d)
            want = (B, L, self.cfg.d_model)
        else:                           # SelfAttnV2 projects to lowerdim
            want = (B, self.cfg.lowerdim if self.cfg.attn_version == 2 else self.cfg.d_model)
        if tuple(e.shape) != want:
            raise ValueError("embedding must have shape %r" % (want,))
        return e

    def _expected_len(self, expected_len, rows=None):
        """One key limit per batch row (or per one of ``rows``) as c_int[B] (rows past the given ones: seq_len), or None for None."""
        if expected_len is None:
            return None
        B = self.cfg.batch if rows is None else rows
        arr = np.zeros(B, dtype=np.int32)
        v = np.asarray(expected_len).astype(np.int32).reshape(-1)
        arr[:len(v)] = v
        arr[len(v):] = self.cfg.seq_len
        return (C.c_int * B)(*arr.tolist())

    def _decode_call(self, entry, embedding, expected_len, n_valid, sos, eos, max_steps, *extra):
        """One reconstruction call of the C ABI (``entry``; ``extra``: its arguments between out_len and the stream) ->
        (the n_valid decoded rows on the host: int32 tokens or float32 stroke-5 rows, their column count)."""
        B = self.cfg.batch
        e = self._decode_embedding(embedding)
        lim = self._expected_len(expected_len)
        if self.cfg.continuous:
            out = torch.zeros(B, max_steps + 1, 5, dtype=torch.float32, device=self.device)
        else:
            out = torch.zeros(B, max_steps + 1, dtype=torch.int64, device=self.device)
        n_out = C.c_int(0)
        self._enter()
        try:
            _lib.call(entry, self.handle, None if e is None else self._p(e), lim, n_valid, int(sos), int(eos), max_steps,
                      self._p(out), C.byref(n_out), *extra, self._stream())
        finally:
            self._leave()
        self.synchronize()
        res = out[:n_valid, :n_out.value].cpu().numpy()
        return (res if self.cfg.continuous else res.astype(np.int32)), n_out.value

    class _Staged:
        """What _stage hands to _forward_backward_staged, and to nothing else: device tensors that may still be the CALLER's own."""
        __slots__ = ("inp", "tar", "labels")

    def _stage(self, inp, tar, labels):
        """caller-side arguments -> device tensors (enqueued on the CALLER's stream: must precede _enter).  Device tensors of the
        caller are NOT cloned here (round 6): the library copies them into its workspace first thing on the engine's stream and
        _forward_backward_staged - the only consumer of the result - makes the caller's stream wait for exactly that copy
        (skf_model_wait_inputs_staged); the two clone kernels per step sat on the caller's stream in front of the hand-over,
        ~19 us of idle GPU at the head of every step."""
        clone = self._step_clones
        st = self._Staged()
        st.inp = self._dev_input(inp, clone)
        st.tar = st.inp if tar is None else self._dev_input(tar, clone)
        st.labels = self._dev_tokens(labels, clone, self.cfg.n_classes if self.cfg.do_classification and self.cfg.lowerdim else None,
                                     "class label")
        return st

    def _forward_backward_staged(self, st):
        self._hold(st.inp, st.tar, st.labels)
        _lib.call("skf_model_forward_backward", self.handle, self._p(st.inp), self._p(st.tar), self._ld(st.tar), self._p(st.labels),
                  self._stream())
        # the caller may refill its device tensors as soon as the staging copy has read them: its stream waits for that copy only
        _lib.call("skf_model_wait_inputs_staged", self.handle, torch.cuda.current_stream(self.device).cuda_stream)

    def forward_backward(self, inp, tar, labels):
        self._refuse_live("forward_backward")
        staged = self._stage(inp, tar, labels)
        self._enter()
        try:
            self._forward_backward_staged(staged)
        finally:
            self._leave()

    def grad_buckets(self):
        """[(offset, count)] slices of the flat gradient buffer in the order they become final during backward."""
        off, cnt = (C.c_size_t * 2)(), (C.c_size_t * 2)()
        n = int(self.lib.skf_model_grad_buckets(self.handle, 2, off, cnt))      # returns the count (negative = error)
        if n <= 0:
            _lib.check(n if n < 0 else -1, "skf_model_grad_buckets")
        return [(int(off[i]), int(cnt[i])) for i in range(n)]

    def apply_gradients(self, bucketed=None, micro=None):
        """optimizer.apply_gradients (models/sketchformer.py:348).  Data parallel: every gradient bucket is all-reduced
        on a communication stream as soon as backward has finished it (bucket 0 = decoder part, overlaps the encoder
        backward; bucket 1 overlaps the optimizer sweep of bucket 0), then the optimizer runs per bucket with the 1/W
        factor fused.  ``bucketed=True`` forces that schedule without a process group (single-GPU test of the plumbing).
        With ``set_gradient_clip`` configured the gradients are all-reduced the same way, but the engine's stream then waits for
        ALL buckets and issues one skf_model_apply_gradients_clipped: a norm needs every gradient before the first update, so the
        overlap of bucket 1's all-reduce with bucket 0's sweep is given up (the overlap with the backward stays).
        ``micro`` is set by the accumulation path alone (train_step, flush_accumulation, a caller's CLOSE): `grads` then holds the sum of that many micro-batch
        gradients, written by a launch on the engine's stream behind the backward - the factor becomes 1 / (world_size * micro)
        and the communication stream waits for the engine's stream instead of for the per-bucket events of the last backward."""
        from . import parallel
        self._refuse_live("apply_gradients")
        if bucketed is None:
            bucketed = self.world_size > 1 and self.dp_mode == "bucketed"
        sweep = "skf_model_apply_gradients" if self._clip is None else "skf_model_apply_gradients_clipped"
        self._enter()
        try:
            if not bucketed:
                scale = 1.0
                if self.world_size > 1:       # one all-reduce of the whole flat buffer, ordered after backward on the step's stream
                    with torch.cuda.stream(self.stream):
                        scale = parallel.allreduce_flat_gradients(self._grads, self.pg)
                if micro is not None:
                    scale = 1.0 / (max(self.world_size, 1) * micro)
                _lib.call(sweep, self.handle, scale, self._stream())
                self._update_weight_average()
                return
            if self._comm is None:
                self._comm = torch.cuda.Stream(device=self.device)
            buckets = self.grad_buckets()
            scale = 1.0 / (max(self.world_size, 1) * (micro or 1))
            works = []
            if self.cfg.use_graph or micro is not None:
                # a step replayed from a hipGraph records no per-bucket events (one bucket): the communication stream must be
                # ordered after the whole captured forward/backward, or the all-reduce would race with the gradient writes.
                # An accumulated gradient is finished by the closing launch on the engine's stream, behind every bucket event
                self._comm.wait_stream(self.stream)
            for i, (off, cnt) in enumerate(buckets):
                if micro is None:
                    _lib.call("skf_model_wait_grad_bucket", self.handle, i, C.c_void_p(self._comm.cuda_stream))
                with torch.cuda.stream(self._comm):
                    works.append(parallel.allreduce_bucket(self._grads[off:off + cnt], self.pg))
            for i, (off, cnt) in enumerate(buckets):
                with torch.cuda.stream(self.stream):
                    if works[i] is not None:
                        works[i].wait()                      # engine stream waits for this bucket's all-reduce
                    else:
                        self.stream.wait_stream(self._comm)
                if self._clip is None:
                    _lib.call("skf_model_apply_gradients_range", self.handle, off, cnt, scale, int(i == len(buckets) - 1), self._stream())
            if self._clip is not None:       # a norm needs every gradient before the first update: ALL buckets, then the one clipped call
                _lib.call(sweep, self.handle, scale, self._stream())
            self._update_weight_average()
        finally:
            self._leave()

    def set_gradient_clip(self, clipnorm=None, global_clipnorm=None, clipvalue=None, skip_nonfinite=False, monitor=False):
        """tf.keras optimizers' clipnorm (every variable's gradient scaled to an L2 norm of at most clipnorm), global_clipnorm (all
        gradients by one factor, to a global norm of at most global_clipnorm) or clipvalue (every element clamped to +-clipvalue):
        at most one of them (``check_gradient_clip``).  skip_nonfinite: a step whose gradient holds an inf or NaN leaves parameters,
        moments and ``iterations`` untouched and is counted (tf LossScaleOptimizer's rule).  monitor: compute the norms even when
        nothing else needs them (``gradient_stats``).  Everything is decided on the device: a configured step is a constant launch
        sequence without a host sync (skf_model_apply_gradients_clipped; two norm launches, the segment scale in per-variable
        mode, one sweep).  Under data parallelism every rank computes the same norms from the same all-reduced buffer (1/world_size
        enters as a factor on the norms): no extra collective.  Nothing set = the unconfigured step, launch for launch."""
        mode, threshold, cv = check_gradient_clip(clipnorm, global_clipnorm, clipvalue)
        on = bool(mode or cv or skip_nonfinite or monitor)
        self.synchronize()
        if not on:
            _lib.call("skf_model_set_gradient_clip", self.handle, 0, 0.0, 0.0, 0, 0, None, 0)
            self._clip = None
            return
        E = len(self.entries)
        nbytes = int(self.lib.skf_model_clip_workspace_bytes(C.byref(self.cfg)))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-ws.data_ptr()) % 256
        torch.cuda.synchronize(self.device)
        _lib.call("skf_model_set_gradient_clip", self.handle, mode, threshold, cv, int(bool(skip_nonfinite)), int(bool(monitor)),
                  C.c_void_p(ws.data_ptr() + off), nbytes)
        stats = ws[off:off + 4 * (8 + 2 * E)].view(torch.float32)      # the stats words lead the workspace (include/skf.h)
        self._clip = {"mode": mode, "threshold": threshold, "clipvalue": cv, "skip_nonfinite": bool(skip_nonfinite),
                      "monitor": bool(monitor), "workspace": ws, "stats": stats,
                      "norms": bool(mode or skip_nonfinite or monitor)}

    def _clip_stats(self):
        if self._clip is None:
            raise _lib.SkfError("no gradient clip / monitor is configured (set_gradient_clip)")
        self._publish()
        return self._clip["stats"]

    def gradient_stats(self):
        """The statistics of the last configured step (host sync): dict(global_norm, scale, nonfinite, skipped, skipped_total,
        norms {variable: L2 norm of its gradient}, scales {variable: the factor applied to it}).  Norms are those of the gradient
        as the optimizer saw it (after the all-reduce, times 1/world_size), before clipping; with clipvalue alone no norm is
        computed and the norm fields stay 0."""
        from . import ops
        st = ops.read_segment_stats(self._clip_stats(), len(self.entries))
        names = [e["name"] for e in self.entries]
        st["norms"] = dict(zip(names, (float(x) for x in st["norms"])))
        st["scales"] = dict(zip(names, (float(x) for x in st["scales"])))
        return st

    def gradient_report(self):
        """Per variable: {'grad_norm', 'weight_norm', 'ratio'} - the gradient norm of the last configured step, the L2 norm of the
        variable itself (the same two launches over ``params``) and grad_norm / weight_norm (inf for an all-zero variable with a
        gradient, 0 when both are zero).  One extra read-back."""
        from . import ops
        stats = self._clip_stats()
        if getattr(self, "_report_plan", None) is None:
            self._report_plan = ops.segment_plan(self.entries, self.device)
        with torch.cuda.stream(self.stream):
            wst = ops.segment_norms(self._params, self._report_plan)
            both = torch.cat([stats, wst])
        self.stream.synchronize()
        E = len(self.entries)
        g = ops.read_segment_stats(both[:8 + 2 * E], E)
        w = ops.read_segment_stats(both[8 + 2 * E:], E)
        out = {}
        for i, e in enumerate(self.entries):
            gn, wn = float(g["norms"][i]), float(w["norms"][i])
            out[e["name"]] = {"grad_norm": gn, "weight_norm": wn, "ratio": gn / wn if wn else (float("inf") if gn else 0.0)}
        return {"global_norm": g["global_norm"], "weight_global_norm": w["global_norm"], "scale": g["scale"],
                "skipped_total": g["skipped_total"], "variables": out}

    def train_step(self, inp, labels, tar=None):
        """model_trainer(inp, tar, lab) (models/sketchformer.py:325-349); no host sync."""
        self._refuse_live("train_step")
        staged = self._stage(inp, tar, labels)       # host-to-device copies of the batch go to the caller's stream FIRST:
        self._enter()                                # the hand-over below is what orders the step behind them
        try:
            self._forward_backward_staged(staged)
            if self._accum is None:
                self.apply_gradients()
            else:
                self._accumulate_micro_step()
        finally:
            self._leave()

    # ---- gradient accumulation: k micro-batches, one optimizer step (include/skf.h: skf_model_accumulate_gradients)
    def set_gradient_accumulation(self, steps):
        """``steps`` = k micro-batches per optimizer step (``check_gradient_accumulation``); 1 switches everything off and train_step
        issues the launches it always issued.  With k > 1 train_step runs forward and backward, sums the gradient into an
        accumulation buffer of ``n_floats`` floats (allocated here) and returns - no all-reduce, no bucket wait, no sweep - until
        the k-th call, which closes the sum into ``grads`` and runs ``apply_gradients`` with 1 / (world_size * k): clipping, the
        norms, skip_nonfinite, ``iterations``, the learning-rate schedule and ``skipped_total`` all see ONE optimizer step on the
        mean gradient of k * batch * world_size rows.  Every micro-step draws its own dropout masks.  The running metrics go on
        accumulating per micro-batch.  Pending micro-batches of an earlier setting are discarded (``reset_accumulation``)."""
        k = check_gradient_accumulation(steps)
        self.reset_accumulation()
        self.synchronize()
        if k == 1:
            self._accum = None
            return
        self._accum = {"k": k, "acc": torch.empty(self.n_floats, dtype=torch.float32, device=self.device), "pending": 0}
        torch.cuda.current_stream(self.device).synchronize()      # (the allocation is the caller stream's, the launches the engine's)

    @property
    def accumulation_pending(self):
        """micro-batches summed so far into the open optimizer step (0 .. k-1; 0 without accumulation)"""
        return 0 if self._accum is None else self._accum["pending"]

    def accumulate_gradients(self, phase):
        """One phase of skf_model_accumulate_gradients behind a ``forward_backward`` (what train_step issues; by hand for a caller
        that drives the pieces itself): _lib.ACCUM_FIRST acc = grads, ACCUM_ADD acc += grads, ACCUM_CLOSE grads = acc + grads - then
        ``apply_gradients(micro=j)`` for the j micro-batches summed - and ACCUM_RESET.  Keeps ``accumulation_pending`` in step."""
        a = self._accum
        if a is None:
            raise _lib.SkfError("no gradient accumulation is configured (set_gradient_accumulation)")
        self._enter()
        try:
            _lib.call("skf_model_accumulate_gradients", self.handle, self._p(a["acc"]), int(phase), self._stream())
            a["pending"] = {_lib.ACCUM_FIRST: 1, _lib.ACCUM_ADD: a["pending"] + 1}.get(int(phase), 0)
        finally:
            self._leave()

    def _accumulate_micro_step(self):
        """behind a forward_backward: sum this micro-batch, and close the optimizer step if it is the k-th"""
        a = self._accum
        if a["pending"] < a["k"] - 1:
            self.accumulate_gradients(_lib.ACCUM_FIRST if a["pending"] == 0 else _lib.ACCUM_ADD)
            return
        micro = a["pending"] + 1
        self.accumulate_gradients(_lib.ACCUM_CLOSE)      # grads = acc + grads, micro = 0
        self.apply_gradients(micro=micro)

    def flush_accumulation(self):
        """Apply what is pending as an optimizer step of its own: j < k micro-batches with 1 / (world_size * j) (the end of an epoch
        whose batch count is no multiple of k).  Nothing pending: nothing happens.  Collective under data parallelism."""
        from . import ops
        a = self._accum
        if a is None or a["pending"] == 0:
            return
        self._enter()
        try:
            with torch.cuda.stream(self.stream):       # grads = acc (the last micro-batch is already part of it), micro = 0
                ops.grad_accumulate(self._grads, a["acc"], None, self._state, _lib.MICRO_ZERO)
            micro, a["pending"] = a["pending"], 0
            self.apply_gradients(micro=micro)
        finally:
            self._leave()

    def reset_accumulation(self):
        """Discard the pending micro-batches (a restored checkpoint carries none): the next train_step opens a new optimizer step."""
        if self._accum is None:
            return
        self.accumulate_gradients(_lib.ACCUM_RESET)

    # ---- weight averaging: an exponential moving average of `params` for evaluation (include/skf.h: skf_model_set_weight_average)
    def set_weight_average(self, decay=None, num_updates=False):
        """tf.train.ExponentialMovingAverage(decay, num_updates=optimizer.iterations if num_updates else None) over the flat parameter
        buffer, without zero-debias.  Allocates the shadow (``n_floats`` floats, ``weight_average``) and starts it at ``params`` -
        tf's rule.  From then on ``apply_gradients`` - plain, clipped, bucketed, and under accumulation the one that closes an
        optimizer step - ends with one more launch, shadow -= (shadow - params) * (1 - d); d = decay, or with ``num_updates``
        min(decay, (1 + n) / (10 + n)) for n = ``iterations`` after the step, read by the kernel.  A step that skip_nonfinite skips
        leaves the shadow untouched.  Under data parallelism every rank averages the same parameters: no collective.
        ``decay=None`` switches averaging off and frees the shadow; an unconfigured engine issues the launches it always issued."""
        if self.average_live:
            raise _lib.SkfError("the weight average is live in `params` (swap_weight_average): swap back before reconfiguring it")
        self.synchronize()
        if decay is None:
            _lib.call("skf_model_set_weight_average", self.handle, None, 0.0, 0)
            self._avg = None
            return
        d = check_weight_average(decay)
        shadow = torch.empty(self.n_floats, dtype=torch.float32, device=self.device)
        _lib.call("skf_model_set_weight_average", self.handle, self._p(shadow), d, int(bool(num_updates)))
        self._avg = {"decay": d, "num_updates": bool(num_updates), "shadow": shadow, "live": False}
        self.reset_weight_average()

    @property
    def average_live(self):
        """True between two ``swap_weight_average``: `params` holds the average, the shadow the raw weights; training is refused"""
        return self._avg is not None and self._avg["live"]

    def _refuse_live(self, what):
        if self._avg is not None and self._avg["live"]:
            raise _lib.SkfError("%s: the weight average is live in `params` (swap_weight_average / averaged_weights): swap back before "
                                "training" % what)

    def _need_average(self):
        if self._avg is None:
            raise _lib.SkfError("no weight average is configured (set_weight_average)")
        return self._avg

    def _update_weight_average(self):
        """the tail of apply_gradients: one launch on the engine's stream behind the sweep; nothing without averaging"""
        if self._avg is not None:
            _lib.call("skf_model_update_weight_average", self.handle, self._stream())

    def reset_weight_average(self):
        """shadow = params: the average starts over from the current weights (what a fresh tf shadow variable holds)"""
        a = self._need_average()
        self._refuse_live("reset_weight_average")
        self._enter()
        try:
            with torch.cuda.stream(self.stream):
                a["shadow"].copy_(self._params)
        finally:
            self._leave()

    def swap_weight_average(self):
        """params <-> shadow in place, one launch on the engine's stream; toggles ``average_live``.  Every forward rebuilds its weight
        images from `params`: after the swap every inference entry (forward, encode, the decoders, score) runs on the average."""
        a = self._need_average()
        self._enter()
        try:
            _lib.call("skf_model_swap_weight_average", self.handle, self._stream())
            a["live"] = bool(self.lib.skf_model_weight_average_live(self.handle))
        finally:
            self._leave()

    def averaged_weights(self):
        """Context manager: the body runs with the averaged weights in `params`; the swap back happens also when the body raises.
        Entered while the average is already live it changes nothing and leaves it live."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self._need_average()
            swapped = not self.average_live
            if swapped:
                self.swap_weight_average()
            try:
                yield self
            finally:
                if swapped and self.average_live:
                    self.swap_weight_average()
        return scope()

    def buffer(self, name):
        """(rows, cols) view of an internal activation.  fp32 models: a float32 view of the workspace; bf16 models keep
        most activations in bf16 (row pitch padded to 8 elements): a bfloat16 view - call .float() for arithmetic."""
        ptr, rows, cols, ld, is16 = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.call("skf_model_buffer_info", self.handle, name.encode(), C.byref(ptr), C.byref(rows), C.byref(cols), C.byref(ld),
                  C.byref(is16))
        esz = 2 if is16.value else 4
        lo = self._ws_ptr - self.workspace.data_ptr()
        ws = self.workspace[lo:lo + self._ws_bytes].view(torch.bfloat16 if is16.value else torch.float32)
        off = (ptr.value - self._ws_ptr) // esz
        return ws[off:off + rows.value * ld.value].view(rows.value, ld.value)[:, :cols.value]

    def step_metrics(self):
        """This step's five scalars (host sync)."""
        m = self.metrics[:5].cpu().numpy()
        return dict(zip(METRIC_NAMES, (float(x) for x in m)))

    def running_metrics(self):
        """Keras running metrics (never reset during train(), core/models.py:183-197)."""
        m = self.metrics.cpu().numpy()
        return {n: float(m[8 + i] / m[16 + i]) if m[16 + i] else 0.0 for i, n in enumerate(METRIC_NAMES)}

    def reset_metrics(self):
        self.metrics.zero_()

    def fold_metric_accumulators_into_rank0(self):
        """Data parallel, before a checkpoint: the running-metric (sum, count) accumulators of all ranks are summed into rank
        0's buffer and zeroed elsewhere (collective).  Later reads still sum over the ranks, so nothing is counted twice, and
        the file rank 0 writes carries every rank's history (restore: rank 0 loads it, the others start from zero)."""
        if self.world_size <= 1:
            return
        self._enter()               # after whatever the caller's stream wrote into the buffer (load_state_dict); marks it unpublished
        try:
            with torch.cuda.stream(self.stream):
                acc = torch.cat([self._metrics[8:13], self._metrics[16:21]]).contiguous()
                torch.distributed.all_reduce(acc, op=torch.distributed.ReduceOp.SUM, group=self.pg)
                if self.rank == 0:
                    self._metrics[8:13], self._metrics[16:21] = acc[:5], acc[5:]
                else:
                    self.zero_metric_accumulators()
        finally:
            self._leave()

    def zero_metric_accumulators(self):
        self._enter()
        try:
            with torch.cuda.stream(self.stream):
                self._metrics[8:13] = 0.0
                self._metrics[16:21] = 0.0
        finally:
            self._leave()

    def metrics_snapshot(self):
        """Device copy of the 32 metric floats as they stand after the steps queued so far (no host sync): what
        ``train_on_batch`` hands back; ``resolve_metrics`` turns a list of them into floats with ONE read-back."""
        with torch.cuda.stream(self.stream):
            if self._clip is None:
                snap = self._metrics.clone()
            else:      # + the 8 leading statistics words (bit copies: three of them are integers), still one read-back at log time
                snap = torch.cat([self._metrics, self._clip["stats"][:8]])
        return snap

    def resolve_metrics(self, snaps, reduce=True):
        """[snapshot] -> [running-metric dict].  One device->host copy for the whole list; under data parallelism the
        (sum, count) accumulators are summed over the ranks first (all-reduce only when metrics are read),
        so every rank must call this with the same number of snapshots.  reduce=False: this rank's own running values,
        no collective (what a rank-specific read such as ``if rank == 0: log(res['total_loss'])`` gets)."""
        if not snaps:
            return []
        with torch.cuda.stream(self.stream):
            m = torch.stack(list(snaps))
            if self.world_size > 1 and reduce:
                acc = torch.cat([m[:, 8:13], m[:, 16:21]], dim=1).contiguous()
                torch.distributed.all_reduce(acc, op=torch.distributed.ReduceOp.SUM, group=self.pg)
                m = m.clone()
                m[:, 8:13], m[:, 16:21] = acc[:, :5], acc[:, 5:]
        self.stream.synchronize()
        rows = m.cpu().numpy()
        out = [{n: float(r[8 + i] / r[16 + i]) if r[16 + i] else 0.0 for i, n in enumerate(METRIC_NAMES)} for r in rows]
        if rows.shape[1] > 32:      # snapshots of a configured engine carry the statistics words (metrics_snapshot)
            for res, r in zip(out, rows):
                res["grad_norm"] = float(r[32])
                res["skipped_steps"] = float(np.ascontiguousarray(r[32:40]).view(np.uint32)[4])
        return out

    def assert_replicas_equal(self):
        """Data parallelism keeps W copies of the parameters / optimizer state in step only if they start equal: compare
        every rank's flat buffers with rank 0's (one broadcast each) and raise on any difference."""
        if self.world_size <= 1:
            return
        import torch.distributed as dist
        src = dist.get_global_rank(self.pg, 0) if self.pg is not None else 0
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        for name in ("params", "adam_m", "adam_v") + (("weight_average",) if self._avg is not None else ()):
            mine = getattr(self, name)
            ref = mine.clone()
            dist.broadcast(ref, src=src, group=self.pg)
            if not torch.equal(ref, mine):
                bad += 1
        its = self.state[:1].clone()
        dist.broadcast(its, src=src, group=self.pg)
        if int(its.item()) != self.iterations:
            bad += 1
        dist.all_reduce(bad, op=dist.ReduceOp.SUM, group=self.pg)
        if int(bad.item()):
            raise _lib.SkfError("data-parallel replicas differ at start (parameters / optimizer state / weight average / iterations): "
                                "every rank must build the model with the same init_seed and restore the same checkpoint")

    @property
    def iterations(self):
        return int(self.state[0].item())
