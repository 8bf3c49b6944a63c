"""``sketch-transformer-tf2`` on MI355X: the plugin surface of models/sketchformer.py (:17-365) over
TrainEngine (the C-ABI HIP train step).  Same registry name, hparams, ctor, ``train_on_batch`` contract
and metric names; the arithmetic runs in libskf.so - there is no CPU / eager fallback.
"""
import zlib
from collections.abc import Mapping

import numpy as np

from .. import builders
from ..core.models import BaseModel
from .evaluation_mixin import TransformerMetricsMixin
from ..utils.hparams import HParams


class DeferredMetrics(Mapping):
    """What ``train_on_batch`` returns: the reference's {metric name: float} dict (models/sketchformer.py:351-359), read
    back from the device only when somebody looks.  The reference pays one host sync per step for ``.numpy()``
    (builders/keras_metrics.py:41-42); here the step only snapshots the 32 device floats, ``BaseModel.train`` resolves
    all pending snapshots with ONE copy when it prints (``log_every``), and a caller that indexes / iterates the mapping
    right away gets the same floats the reference would have returned (one sync, like the reference).  Under data
    parallelism ``resolve_all`` (what ``BaseModel.train`` calls on EVERY rank) all-reduces the (sum, count) accumulators;
    indexing / iterating / printing a single result never runs a collective - it reads this rank's own running values, so a
    rank-specific read (``if rank == 0: log(res['total_loss'])``) cannot deadlock."""

    def __init__(self, engine, snapshot, drop):
        self._engine, self._snap, self._drop, self._vals = engine, snapshot, drop, None

    def resolve_with(self, vals):
        self._vals = {k: v for k, v in vals.items() if k not in self._drop}
        self._snap = None

    def _resolved(self):
        if self._vals is None:
            self.resolve_with(self._engine.resolve_metrics([self._snap], reduce=False)[0])
        return self._vals

    @staticmethod
    def resolve_all(pending):
        """One read-back (and, data parallel, one all-reduce) for a list of unresolved results of the same engine."""
        todo = [p for p in pending if p._vals is None]
        if todo:
            for p, vals in zip(todo, todo[0]._engine.resolve_metrics([p._snap for p in todo])):
                p.resolve_with(vals)

    def __getitem__(self, k):
        return self._resolved()[k]

    def __iter__(self):
        return iter(self._resolved())

    def __len__(self):
        return len(self._resolved())

    def __repr__(self):
        return repr(self._resolved())


def score_in_chunks(inp_seq, tar_seq, seq_len, batch, eos, score_chunk):
    """The host side of ``Transformer.score``, free of the device.  inp_seq: (n, seq_len) model-ready token rows (a single row, or
    the (n, seq_len, 1) token columns of the file loaders, are accepted); tar_seq: None (= inp_seq) or n rows of seq_len or
    seq_len + 1 columns - the shape predict / sample / beam_search return - of which the forward consumes the first seq_len.
    The rows go to ``score_chunk(inp (batch, seq_len), tar (batch, seq_len), m)`` in consecutive chunks of ``batch`` rows, the last one
    zero-padded, m of them valid; it returns (tok_logp (m, seq_len - 1), tok_rank, seq_logp (m,), seq_len (m,)) host arrays.
    Returns {'logp': (n,), 'length': (n,), 'token_logp': (n, seq_len - 1), 'rank': (n, seq_len - 1),
    'perplexity': exp(-logp / max(length, 1)), 'complete': (n,) bool - the row's EOS lies inside the scored window tar[:, 1:seq_len]}.
    A row that runs past the window is scored on what fits and flagged through 'complete', not rejected."""
    def rows(x, what, widths):
        x = np.asarray(x)
        if x.ndim == 1:
            x = x[None]
        if x.ndim == 3 and x.shape[-1] == 1:
            x = x[..., 0]
        if x.ndim != 2 or x.shape[1] not in widths:
            raise ValueError("%s must hold rows of %s tokens (got shape %r)" % (what, " or ".join(str(w) for w in widths), x.shape))
        return x.astype(np.int64)
    L, B = int(seq_len), int(batch)
    inp = rows(inp_seq, "inp_seq", (L,))
    tar = inp if tar_seq is None else rows(tar_seq, "tar_seq", (L, L + 1))[:, :L]
    n = len(inp)
    if n == 0:
        raise ValueError("no sequence given")
    if len(tar) != n:
        raise ValueError("tar_seq must hold one row per row of inp_seq (got %d and %d)" % (len(tar), n))
    parts = []
    for i in range(0, n, B):
        m = min(B, n - i)
        pi, pt = np.zeros((B, L), np.int64), np.zeros((B, L), np.int64)
        pi[:m], pt[:m] = inp[i:i + m], tar[i:i + m]
        parts.append([np.asarray(a)[:m] for a in score_chunk(pi, pt, m)])
    token_logp, rank, logp, length = (np.concatenate([p[k] for p in parts], axis=0) for k in range(4))
    with np.errstate(over="ignore"):
        perplexity = np.exp(-logp.astype(np.float64) / np.maximum(length, 1))
    return {'logp': logp, 'length': length, 'token_logp': token_logp, 'rank': rank, 'perplexity': perplexity,
            'complete': (tar[:, 1:L] == eos).any(axis=1)}


class Transformer(BaseModel, TransformerMetricsMixin):
    name = 'sketch-transformer-tf2'
    quick_metrics = ['recon_loss', 'recon_acc', 'class_loss', 'class_acc', 'total_loss']
    slow_metrics = ["sketch-reconstruction", "val-clas-acc", "tsne", "tsne-predicted"]

    @classmethod
    def specific_default_hparams(cls):
        """models/sketchformer.py:25-53 (names, defaults and types unchanged)."""
        return HParams(
            num_layers=4, d_model=128, dff=512, num_heads=8, dropout_rate=0.1,
            lowerdim=256, attn_version=1,
            do_classification=True, class_weight=1.0, class_buffer_layers=0, class_dropout=0.1,
            do_reconstruction=True, recon_weight=1.0, blind_decoder_mask=True,
            is_training=True, optimizer='Adam', lr=0.01, lr_scheduler='WarmupDecay', warmup_steps=10000,
        )

    def __init__(self, hps, dataset, out_dir, experiment_id, device=None, process_group=None, init_seed=0):
        self.losses_manager = builders.losses.LossManager()
        self.metrics_manager = builders.keras_metrics.MetricManager()
        self.vocab_size = dataset.tokenizer.VOCAB_SIZE if not dataset.hps['use_continuous_data'] else None
        self.seq_len = dataset.hps['max_seq_len']
        self._device, self._pg, self._init_seed = device, process_group, init_seed
        super().__init__(hps, dataset, out_dir, experiment_id, process_group=process_group)

    def build_model(self):
        from .. import engine
        h = self.hps
        if h['optimizer'].lower() not in ('adam', 'sgd'):
            raise ValueError("optimizer=%r: the reference builds Adam or SGD (models/sketchformer.py:120-126)" % h['optimizer'])
        # models/sketchformer.py:76-108: decoder / losses / metrics are only registered for the heads that exist
        self._has_cls = bool(h['lowerdim']) and bool(h['do_classification'])
        if h['do_classification'] and not h['lowerdim']:
            raise ValueError("do_classification needs lowerdim > 0 (models/sketchformer.py:96-108: the class head lives "
                             "inside the bottleneck block; the reference fails on the unregistered 'class' loss)")
        if h['do_reconstruction']:
            if self.dataset.hps['use_continuous_data']:
                self.losses_manager.add_continuous_reconstruction_loss('recon', weight=h['recon_weight'])
                self.metrics_manager.add_mean_metric('recon_loss')
            else:
                self.losses_manager.add_reconstruction_loss('recon', weight=h['recon_weight'])
                self.metrics_manager.add_mean_metric('recon_loss')
                self.metrics_manager.add_sparse_categorical_accuracy('recon_acc')
        if self._has_cls:
            self.losses_manager.add_sparse_categorical_crossentropy('class', weight=h['class_weight'])
            self.metrics_manager.add_mean_metric('class_loss')
            self.metrics_manager.add_sparse_categorical_accuracy('class_acc')
        self.metrics_manager.add_mean_metric('total_loss')
        # WarmupDecay is built with warmup_steps=5000 whatever the hparams say (models/sketchformer.py:113-114)
        self.learning_rate = (builders.schedulers.WarmupDecay(h['d_model'], warmup_steps=5000)
                              if h['lr_scheduler'].lower() in ('warmupdecay', 'warmup-decay') else None)
        cfg = engine.make_config(
            batch=h['batch_size'], seq_len=self.seq_len, d_model=h['d_model'], num_heads=h['num_heads'], dff=h['dff'],
            num_layers=h['num_layers'], vocab_size=self.vocab_size or 0, n_classes=self.dataset.n_classes,
            lowerdim=h['lowerdim'], attn_version=h['attn_version'], continuous=self.dataset.hps['use_continuous_data'],
            blind_decoder_mask=h['blind_decoder_mask'], dropout_rate=h['dropout_rate'], recon_weight=h['recon_weight'],
            class_weight=h['class_weight'], lr_scheduler=h['lr_scheduler'], lr=h['lr'], use_graph=False,
            optimizer=h['optimizer'], class_buffer_layers=h['class_buffer_layers'], class_dropout=h['class_dropout'],
            do_classification=h['do_classification'], do_reconstruction=h['do_reconstruction'],
            # dropout key = hash(seed, iterations): the seed differs per experiment id and per rank (ranks must
            # draw independent masks, or W ranks at B rows are not one step at W*B rows); the weight init seed does NOT
            # depend on the rank - replicas start identical (checked below)
            seed=(zlib.crc32(str(self.experiment_id).encode()) + 0x9e3779b1 * self.rank) & 0xffffffff)
        self.engine = engine.TrainEngine(cfg, device=self._device, init_seed=self._init_seed, process_group=self._pg)
        self.engine.assert_replicas_equal()
        self.trainable_variables = [e["name"] for e in self.engine.entries]
        drop = set()
        if self.dataset.hps['use_continuous_data'] or not h['do_reconstruction']:
            drop.add('recon_acc')
        if not h['do_reconstruction']:
            drop.add('recon_loss')
        if not self._has_cls:
            drop.update(('class_loss', 'class_acc'))
        self._dropped_metrics = drop

    # ---- the train step (models/sketchformer.py:351-359)
    def train_on_batch(self, batch):
        data, labels = batch
        self.engine.train_step(data, labels)
        # the Keras running metrics of this step, as a mapping that is read back lazily (no host sync here)
        return DeferredMetrics(self.engine, self.engine.metrics_snapshot(), self._dropped_metrics)

    def prepare_for_start_of_epoch(self):
        pass

    def prepare_for_end_of_epoch(self):
        self.engine.reset_metrics()

    # ---- inference API (models/sketchformer.py:162-311); inputs are padded to the engine's batch size
    def _pad_batch(self, x):
        x = np.asarray(x)
        if x.ndim == (2 if self.engine.cfg.continuous else 1):
            x = x[None]
        n, B = x.shape[0], self.engine.cfg.batch
        if n > B:
            raise ValueError("at most batch_size=%d sequences per call" % B)
        pad = np.zeros((B,) + x.shape[1:], dtype=np.float32 if self.engine.cfg.continuous else np.int64)
        if self.engine.cfg.continuous:
            pad[..., 4] = 1.0                      # stroke-5 padding rows
        pad[:n] = x
        return pad, n

    def encode_from_seq(self, inp_seq):
        pad, n = self._pad_batch(inp_seq)
        self.engine.encode(pad)
        self.engine.synchronize()
        B = self.engine.cfg.batch
        enc = self.engine.buffer('enc_output').view(B, self.seq_len, -1)[:n].cpu().numpy()
        emb = self.engine.buffer('embedding')[:n].cpu().numpy() if self.hps['lowerdim'] else enc
        return {'enc_output': enc, 'embedding': emb,
                'class': self.engine.buffer('class_probs')[:n].cpu().numpy() if self._has_cls else None}

    def predict_class(self, inp_seq):
        out = self.encode_from_seq(inp_seq)
        if self._has_cls:
            out['class'] = out['class'].argmax(-1).astype(np.int32)
        return out

    def make_dummy_input(self, expected_len, nattn, batch_size):
        """models/sketchformer.py:230-253: fake encoder input, only its padding mask matters (first nattn positions real)."""
        if self.engine.cfg.continuous:
            d = np.zeros((batch_size, self.seq_len, 5), dtype=np.float32)
            d[:, int(nattn):, 4] = 1.0
            return d
        d = np.zeros((batch_size, self.seq_len), dtype=np.float32)
        if expected_len is None:
            d[:, :int(nattn)] = 1.0
        else:
            for b, n in enumerate(np.asarray(nattn).reshape(-1)):
                d[b, :int(n)] = 1.0
        return d

    def predict_from_embedding(self, emb, expected_len=None, with_attn_weights=False):
        """Greedy reconstruction from the bottleneck (models/sketchformer.py:255-311), KV-cached on the device.
        Returns {'recon', 'class', 'attn_weights'}.  attn_weights is None unless with_attn_weights: then the reference's
        dict of the last decoder pass, {'decoder_layer{i}_block1': (n, H, T, T), 'decoder_layer{i}_block2': (n, H, T, seq_len)}
        float32 with T = recon length - 1 (models/sketchformer.py:306).  Opt-in: the evaluation code calls predict on
        whole splits and reads no weights.  A non-blind model needs expected_len for them (ValueError otherwise)."""
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        emb = np.asarray(emb, dtype=np.float32)
        if emb.ndim == (1 if self.hps['lowerdim'] else 2):     # one embedding: (E,) - or (L, d) without a bottleneck
            emb = emb[None]
        n, B = emb.shape[0], self.engine.cfg.batch
        if n > B:
            raise ValueError("at most batch_size=%d embeddings per call" % B)
        pad = np.zeros((B,) + emb.shape[1:], dtype=np.float32)
        pad[:n] = emb
        if self.hps['blind_decoder_mask']:
            expected_len = None                     # "will be ignored if blind_decoder_mask=True"
        if with_attn_weights and expected_len is None and not self.hps['blind_decoder_mask']:
            raise ValueError("attn_weights of a non-blind decoder need expected_len (with nattn = i + 1 the decoded rows "
                             "were masked differently from the reference's last pass)")
        sos, eos = self._sos_eos()
        res = self.engine.greedy_decode(pad, expected_len=expected_len, n_valid=n, sos=sos, eos=eos, with_attn_weights=with_attn_weights)
        recon, weights = res if with_attn_weights else (res, None)
        out = {'recon': recon, 'attn_weights': weights}
        if self._has_cls:
            out['class'] = self.engine.buffer('class_probs')[:n].cpu().numpy().argmax(-1).astype(np.int32)
        return out

    def predict(self, inp_seq, with_attn_weights=False):
        """models/sketchformer.py:201-221.  with_attn_weights: out['attn_weights'] = the decoder's attention weights
        (see predict_from_embedding), else None."""
        out = self.encode_from_seq(inp_seq)
        if self._has_cls:
            out['class'] = out['class'].argmax(-1).astype(np.int32)
        if self.hps['do_reconstruction']:
            x = np.asarray(inp_seq)
            if self.hps['blind_decoder_mask']:
                tlen = None
            elif self.engine.cfg.continuous:
                tlen = np.sum(x[..., -1] != 1, axis=-1).reshape(-1)
            else:
                tlen = np.sum(x > 0, axis=-1).reshape(-1)
            dec = self.predict_from_embedding(out['embedding'], tlen, with_attn_weights=with_attn_weights)
            out['recon'] = dec['recon']
            out['attn_weights'] = dec['attn_weights']
        return out

    def _sos_eos(self):
        """(SOS, EOS) of the dataset's tokenizer; (0, 0) without one."""
        tok = self.dataset.tokenizer
        return (getattr(tok, 'SOS', 0), getattr(tok, 'EOS', 0)) if tok is not None else (0, 0)

    def _decode_in_chunks(self, rows, decode):
        """Reconstructions of any number R of embeddings (device tensor, one per row) in consecutive chunks of batch_size rows.  The
        last chunk is zero-padded; ``decode(chunk, i, m)`` gets the batch_size rows that start at row i, m of them valid, and
        returns their (m, T[, 5]) reconstruction, which is zero-padded to seq_len + 1 columns.
        Returns (recon (R, seq_len + 1[, 5]), class (R,) int32 or None)."""
        import torch
        B, L = self.engine.cfg.batch, self.seq_len + 1
        recon, cls = [], []
        for i in range(0, rows.shape[0], B):
            chunk = rows[i:i + B]
            m = chunk.shape[0]
            if m < B:
                chunk = torch.cat([chunk, torch.zeros((B - m,) + tuple(chunk.shape[1:]), dtype=torch.float32, device=chunk.device)], dim=0)
            r = decode(chunk, i, m)
            pad = np.zeros((m, L) + r.shape[2:], dtype=r.dtype)
            pad[:, :r.shape[1]] = r
            recon.append(pad)
            if self._has_cls:
                cls.append(self.engine.buffer('class_probs')[:m].cpu().numpy().argmax(-1).astype(np.int32))
        return np.concatenate(recon, axis=0), (np.concatenate(cls, axis=0) if self._has_cls else None)

    def _beam_chunks(self, rows, decode, B, cls_stride):
        """_decode_in_chunks for beam search: chunks of B = batch_size // beam_width sketches (the last one zero-padded);
        ``decode(chunk, i, m)`` returns ((m, W, T) tokens, extras...), the T axis is zero-padded to seq_len + 1 columns and the extras
        (scores, lengths) are concatenated as they are; the class of sketch r is read from batch row r * cls_stride.
        Returns (recon (R, W, seq_len + 1), [extras...], class (R,) int32 or None)."""
        import torch
        L = self.seq_len + 1
        recon, extras, cls = [], None, []
        for i in range(0, rows.shape[0], B):
            chunk = rows[i:i + B]
            m = chunk.shape[0]
            if m < B:
                chunk = torch.cat([chunk, torch.zeros((B - m,) + tuple(chunk.shape[1:]), dtype=torch.float32, device=chunk.device)], dim=0)
            r, *rest = decode(chunk, i, m)
            pad = np.zeros(r.shape[:2] + (L,), dtype=r.dtype)
            pad[:, :, :r.shape[2]] = r
            recon.append(pad)
            extras = [[x] for x in rest] if extras is None else [a + [x] for a, x in zip(extras, rest)]
            if self._has_cls:
                cls.append(self.engine.buffer('class_probs')[:m * cls_stride:cls_stride].cpu().numpy().argmax(-1).astype(np.int32))
        return (np.concatenate(recon, axis=0), [np.concatenate(a, axis=0) for a in extras],
                (np.concatenate(cls, axis=0) if self._has_cls else None))

    def beam_search_from_embedding(self, emb, beam_width=4, length_alpha=0.0, expected_len=None):
        """The beam_width most likely reconstructions of every embedding (engine.beam_decode; the selection rule is in
        include/skf.h).  emb: any number n of embeddings, a host array or a device tensor (n, E); they are decoded in consecutive
        chunks of batch_size // beam_width sketches.  Every column after a hypothesis's EOS is 0, so a sketch's result depends
        neither on n, nor on its chunk, nor on its neighbours.  expected_len: per embedding, required by a non-blind model.
        Returns {'recon': (n, W, seq_len + 1) int32, best first, 'score': (n, W) float32 sums of log p, 'length': (n, W) int32,
        'class': (n,) int32 or None}."""
        import torch
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.BEAM_NEEDS_TOKENS)
        _engine.check_beam(beam_width, length_alpha)
        eng = self.engine
        _engine.check_beam(beam_width, length_alpha, eng.cfg.vocab_size, eng.cfg.batch)
        W = int(beam_width)
        if not torch.is_tensor(emb):
            emb = torch.as_tensor(np.asarray(emb, dtype=np.float32))
        emb = emb.to(eng.device, dtype=torch.float32)
        if emb.dim() == (1 if self.hps['lowerdim'] else 2):       # one embedding: (E,) - or (L, d) without a bottleneck
            emb = emb[None]
        n = emb.shape[0]
        if n == 0:
            raise ValueError("no embedding given")
        if self.hps['blind_decoder_mask']:
            expected_len = None                                   # "will be ignored if blind_decoder_mask=True"
        elif expected_len is None:
            raise ValueError("beam search of a non-blind decoder needs expected_len")
        else:
            expected_len = np.asarray(expected_len).astype(np.int32).reshape(-1)
            if len(expected_len) != n:
                raise ValueError("expected_len must hold one length per embedding")
        sos, eos = self._sos_eos()
        recon, (score, length), cls = self._beam_chunks(emb, lambda chunk, i, m: eng.beam_decode(
            chunk, expected_len=None if expected_len is None else expected_len[i:i + m], n_valid=m, sos=sos, eos=eos,
            beam_width=W, length_alpha=length_alpha), eng.cfg.batch // W, W)
        ended = np.cumsum(recon[:, :, 1:] == eos, axis=2) > 0     # from the first EOS on (column 0 is the start symbol)
        recon[:, :, 2:][ended[:, :, :-1]] = 0
        return {'recon': recon, 'score': score, 'length': length, 'class': cls}

    def beam_search(self, inp_seq, beam_width=4, length_alpha=0.0):
        """beam_search_from_embedding on the embeddings of inp_seq (any number of model-ready token sequences); the embeddings go
        from the encoder to the decoder on the device.  A non-blind model decodes with its input's length as expected_len, like
        predict."""
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.BEAM_NEEDS_TOKENS)
        _engine.check_beam(beam_width, length_alpha)
        if not self.hps['lowerdim']:
            raise ValueError("beam_search needs lowerdim > 0 (the bottleneck embedding); without one, pass the (n, L, d) encoder "
                             "outputs to beam_search_from_embedding")
        x = np.asarray(inp_seq)
        if x.ndim == 1:
            x = x[None]
        if x.ndim == 3 and x.shape[-1] == 1:
            x = x[..., 0]
        tlen = None if self.hps['blind_decoder_mask'] else np.sum(x > 0, axis=-1).reshape(-1)
        return self.beam_search_from_embedding(self._embed_on_device(x), beam_width=beam_width, length_alpha=length_alpha,
                                               expected_len=tlen)

    def _embed_on_device(self, x):
        """Bottleneck embeddings of any number of model-ready sequences as ONE device (P, E) float32 tensor: encoded in chunks of
        batch_size, every chunk's rows copied out of the 'embedding' buffer device to device."""
        import torch
        x = np.asarray(x)
        B = self.engine.cfg.batch
        z = None
        for i in range(0, len(x), B):
            pad, n = self._pad_batch(x[i:i + B])
            self.engine.encode(pad)
            buf = self.engine.buffer('embedding')          # orders the current stream behind the encode
            if z is None:
                z = torch.empty(len(x), buf.shape[1], dtype=torch.float32, device=buf.device)
            z[i:i + n].copy_(buf[:n])                      # the next encode's hand-over orders it behind this copy
        return z

    def interpolate(self, x_a, x_b, n_steps=10, mode='slerp', decode=True):
        """n_steps embeddings on the way from every sketch of x_a to its partner in x_b (the slerp of
        experiments/interpolations_for_mturk.py:98-108), and their greedy reconstructions.  x_a, x_b: P model-ready sequences
        each (P is not limited by batch_size).  The embeddings stay on the device from the encoder to the decoder
        (ops.interpolate at t = linspace(0, 1, n_steps) in float32).  decode: the P * n_steps rows, pair-major, go through the
        decoder in consecutive chunks of batch_size rows (expected_len=None, like the reference's experiment; the last chunk is
        zero-padded) and every chunk's reconstruction is zero-padded to seq_len + 1 columns - what a row holds after its own
        EOS depends on when its chunk stops, so the chunking is part of the result.
        Returns {'embedding': (P, T, E) float32, 'recon': (P, T, seq_len + 1[, 5]) or None, 'class': (P, T) int32 or None}."""
        import torch
        from .. import ops
        if not self.hps['lowerdim']:
            raise ValueError("interpolate needs lowerdim > 0: without a bottleneck the embedding is the (L, d) encoder output, "
                             "and the reference's slerp of two matrices is not an interpolation")
        if decode and not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        x_a, x_b = np.asarray(x_a), np.asarray(x_b)
        if x_a.shape != x_b.shape or x_a.ndim != (3 if self.engine.cfg.continuous else 2) or len(x_a) == 0:
            raise ValueError("x_a and x_b must hold the same number (>= 1) of model-ready sequences")
        za, zb = self._embed_on_device(x_a), self._embed_on_device(x_b)
        z = ops.interpolate(za, zb, torch.linspace(0, 1, int(n_steps), dtype=torch.float32), mode)
        P, T, E = z.shape
        out = {'embedding': z.cpu().numpy(), 'recon': None, 'class': None}
        if not decode:
            return out
        sos, eos = self._sos_eos()
        recon, cls = self._decode_in_chunks(z.view(P * T, E), lambda chunk, i, m: self.engine.greedy_decode(
            chunk, expected_len=None, n_valid=m, sos=sos, eos=eos))
        out['recon'] = recon.reshape((P, T) + recon.shape[1:])
        if cls is not None:
            out['class'] = cls.reshape(P, T)
        return out

    def sample_from_embedding(self, emb, n_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=0, expected_len=None):
        """n_samples stochastic reconstructions of every embedding: each token is drawn from softmax(logits / temperature) cut to
        its top_k largest entries (0 = off) and then to its nucleus of mass top_p (1 = off) - the selection rule of include/skf.h
        (engine.sample_decode).  emb: any number n of embeddings, a host array or a device tensor (n, E) (it stays where it is).
        Row i * n_samples + s of the replicated batch is draw s of embedding i and uses random stream i * n_samples + s under
        `seed`; the rows are decoded in consecutive chunks of batch_size.  Every column after a row's first EOS is set to 0 (what
        the decoder appends there depends on when the row's chunk stops), so a row depends only on (embedding, parameters, seed,
        its stream id) - not on n, on batch_size or on its neighbours.  expected_len: per embedding, non-blind models only.
        Returns {'recon': (n, n_samples, seq_len + 1) int32, 'class': (n, n_samples) int32 or None}."""
        import torch
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.SAMPLING_NEEDS_TOKENS)
        _engine.check_sampling(temperature, top_k, top_p)
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError("n_samples must be >= 1")
        eng = self.engine
        if not torch.is_tensor(emb):
            emb = torch.as_tensor(np.asarray(emb, dtype=np.float32))
        emb = emb.to(eng.device, dtype=torch.float32)
        if emb.dim() == (1 if self.hps['lowerdim'] else 2):       # one embedding: (E,) - or (L, d) without a bottleneck
            emb = emb[None]
        n = emb.shape[0]
        if n == 0:
            raise ValueError("no embedding given")
        if self.hps['blind_decoder_mask']:
            expected_len = None                                   # "will be ignored if blind_decoder_mask=True"
        if expected_len is not None:
            expected_len = np.repeat(np.asarray(expected_len).astype(np.int32).reshape(-1), n_samples)
            if len(expected_len) != n * n_samples:
                raise ValueError("expected_len must hold one length per embedding")
        sos, eos = self._sos_eos()
        rows = emb.repeat_interleave(n_samples, dim=0)            # (n * n_samples, ...) on the device
        recon, cls = self._decode_in_chunks(rows, lambda chunk, i, m: eng.sample_decode(
            chunk, expected_len=None if expected_len is None else expected_len[i:i + m], n_valid=m, sos=sos, eos=eos,
            temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, stream_ids=np.arange(i, i + m)))
        ended = np.cumsum(recon[:, 1:] == eos, axis=1) > 0        # from the first EOS on (column 0 is the start symbol)
        recon[:, 2:][ended[:, :-1]] = 0
        return {'recon': recon.reshape(n, n_samples, self.seq_len + 1), 'class': None if cls is None else cls.reshape(n, n_samples)}

    def sample(self, inp_seq, n_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        """sample_from_embedding on the embeddings of inp_seq (any number of model-ready token sequences); the embeddings go from
        the encoder to the decoder on the device.  A non-blind model decodes every draw with its input's length as expected_len,
        like predict."""
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.SAMPLING_NEEDS_TOKENS)
        _engine.check_sampling(temperature, top_k, top_p)
        if not self.hps['lowerdim']:
            raise ValueError("sample needs lowerdim > 0 (the bottleneck embedding); without one, pass the (n, L, d) encoder "
                             "outputs to sample_from_embedding")
        x = np.asarray(inp_seq)
        if x.ndim == 1:
            x = x[None]
        if x.ndim == 3 and x.shape[-1] == 1:
            x = x[..., 0]
        tlen = None if self.hps['blind_decoder_mask'] else np.sum(x > 0, axis=-1).reshape(-1)
        return self.sample_from_embedding(self._embed_on_device(x), n_samples=n_samples, temperature=temperature, top_k=top_k,
                                          top_p=top_p, seed=seed, expected_len=tlen)

    def complete_from_embedding(self, emb, prefix, prefix_len=None, expected_len=None, mode='greedy', n_samples=1, temperature=1.0,
                                top_k=0, top_p=1.0, seed=0, beam_width=4, length_alpha=0.0, prefill=True):
        """Sketch completion: the decoder continues the first prefix_len[i] tokens of ``prefix`` row i from embedding i (the rule
        is in include/skf.h: prefix-forced decoding).  emb: any number n of embeddings, a host array or a device tensor (n, E);
        prefix: (n, >= max(prefix_len)) tokens WITHOUT the start symbol; prefix_len=None: each row's tokens before its first EOS or
        PAD.  mode: 'greedy'; 'sample' (n_samples draws per sketch with temperature / top_k / top_p / seed, random streams as in
        sample_from_embedding); 'beam' (the beam_width most likely continuations, ordered like beam_search_from_embedding's).  The
        rows are decoded in chunks like sample_from_embedding / beam_search_from_embedding, and every column after a row's first
        EOS is 0, so a row depends neither on n, nor on its chunk, nor on its neighbours.  expected_len: per embedding, non-blind
        models only (required for 'beam').  prefill: engine.greedy_decode's - the cache rows of the prefixes in num_layers launches
        (it pays when the rows of a chunk share a long prefix) or, False, one position launch per prefix token (the better setting
        for ragged prefixes: the position loop starts at a chunk's SHORTEST prefix); the results are the same bits; beams always step.
        Returns {'recon': (n, seq_len + 1) int32 ['sample': (n, n_samples, seq_len + 1); 'beam': (n, W, seq_len + 1)] with the
        prefix in columns 1 .. prefix_len, 'prefix_len': (n,) int32, 'class': as the mode's own method returns it, and for
        'beam' also 'score' (n, W) float32 = log p(continuation | prefix, embedding) and 'length' (n, W) int32}."""
        import torch
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.COMPLETION_NEEDS_TOKENS)
        if mode not in ('greedy', 'sample', 'beam'):
            raise ValueError("mode must be 'greedy', 'sample' or 'beam' (got %r)" % (mode,))
        eng = self.engine
        if mode == 'sample':
            _engine.check_sampling(temperature, top_k, top_p)
        if mode == 'beam':
            _engine.check_beam(beam_width, length_alpha, eng.cfg.vocab_size, eng.cfg.batch)
        n_samples = int(n_samples) if mode == 'sample' else 1
        if n_samples < 1:
            raise ValueError("n_samples must be >= 1")
        if not torch.is_tensor(emb):
            emb = torch.as_tensor(np.asarray(emb, dtype=np.float32))
        emb = emb.to(eng.device, dtype=torch.float32)
        if emb.dim() == (1 if self.hps['lowerdim'] else 2):       # one embedding: (E,) - or (L, d) without a bottleneck
            emb = emb[None]
        n = emb.shape[0]
        if n == 0:
            raise ValueError("no embedding given")
        sos, eos = self._sos_eos()
        prefix = np.asarray(prefix.cpu() if torch.is_tensor(prefix) else prefix)
        if prefix.ndim == 1:
            prefix = prefix[None]
        if prefix.ndim != 2 or prefix.shape[0] != n:
            raise ValueError("prefix must hold one row of tokens per embedding")
        # the whole set at once: ranges, and the derived lengths (the chunks below pass explicit lengths)
        prefix, plen = _engine.check_prefix(prefix, prefix_len, n, self.seq_len, eng.cfg.vocab_size, eos)
        if self.hps['blind_decoder_mask']:
            expected_len = None                                   # "will be ignored if blind_decoder_mask=True"
        elif expected_len is None:
            if mode == 'beam':
                raise ValueError("beam search of a non-blind decoder needs expected_len")
        else:
            expected_len = np.asarray(expected_len).astype(np.int32).reshape(-1)
            if len(expected_len) != n:
                raise ValueError("expected_len must hold one length per embedding")

        def lim(i, m, rep=1):
            return None if expected_len is None else np.repeat(expected_len, rep)[i:i + m]

        out = {'prefix_len': plen.astype(np.int32)}
        if mode == 'beam':
            W = int(beam_width)
            recon, (score, length), cls = self._beam_chunks(emb, lambda chunk, i, m: eng.beam_complete(
                chunk, prefix[i:i + m], plen[i:i + m], expected_len=lim(i, m), n_valid=m, sos=sos, eos=eos, beam_width=W,
                length_alpha=length_alpha), eng.cfg.batch // W, W)
            ended = np.cumsum(recon[:, :, 1:] == eos, axis=2) > 0
            recon[:, :, 2:][ended[:, :, :-1]] = 0
            out.update(recon=recon, score=score, length=length)
            out['class'] = cls
            return out
        rows = emb.repeat_interleave(n_samples, dim=0)
        rp, rl = np.repeat(prefix, n_samples, axis=0), np.repeat(plen, n_samples)
        if mode == 'sample':
            def decode(chunk, i, m):
                return eng.sample_decode(chunk, expected_len=lim(i, m, n_samples), n_valid=m, sos=sos, eos=eos, temperature=temperature,
                                         top_k=top_k, top_p=top_p, seed=seed, stream_ids=np.arange(i, i + m), prefix=rp[i:i + m],
                                         prefix_len=rl[i:i + m], prefill=prefill)
        else:
            def decode(chunk, i, m):
                return eng.greedy_decode(chunk, expected_len=lim(i, m), n_valid=m, sos=sos, eos=eos, prefix=rp[i:i + m],
                                         prefix_len=rl[i:i + m], prefill=prefill)
        recon, cls = self._decode_in_chunks(rows, decode)
        ended = np.cumsum(recon[:, 1:] == eos, axis=1) > 0        # from the first EOS on (column 0 is the start symbol)
        recon[:, 2:][ended[:, :-1]] = 0
        if mode == 'sample':
            recon = recon.reshape(n, n_samples, self.seq_len + 1)
            cls = None if cls is None else cls.reshape(n, n_samples)
        out.update(recon=recon)
        out['class'] = cls
        return out

    def complete(self, partial_seq, **kw):
        """complete_from_embedding on the embeddings of partial_seq (any number of model-ready token sequences: the part of a sketch
        drawn so far, closed by EOS): the embeddings go from the encoder to the decoder on the device, the prefix of a row is its
        tokens behind the start symbol and before its EOS, and a non-blind model decodes with the partial's length as expected_len, like predict.  kw: mode,
        n_samples, temperature, top_k, top_p, seed, beam_width, length_alpha, prefill."""
        from .. import engine as _engine
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.COMPLETION_NEEDS_TOKENS)
        if not self.hps['lowerdim']:
            raise ValueError("complete needs lowerdim > 0 (the bottleneck embedding); without one, pass the (n, L, d) encoder "
                             "outputs to complete_from_embedding")
        for k in ('prefix', 'prefix_len', 'expected_len'):
            if k in kw:
                raise TypeError("complete() derives %s from partial_seq; use complete_from_embedding to set it" % k)
        x = np.asarray(partial_seq)
        if x.ndim == 1:
            x = x[None]
        if x.ndim == 3 and x.shape[-1] == 1:
            x = x[..., 0]
        tlen = None if self.hps['blind_decoder_mask'] else np.sum(x > 0, axis=-1).reshape(-1)
        # a model-ready row is [SOS] body [EOS] PAD...: the start symbol is the decoder's column 0, the prefix what follows it
        sos = self._sos_eos()[0]
        prefix = np.zeros_like(x)
        for i, row in enumerate(x):
            body = row[1:] if len(row) and row[0] == sos else row
            prefix[i, :len(body)] = body
        return self.complete_from_embedding(self._embed_on_device(x), prefix[:, :self.seq_len], prefix_len=None, expected_len=tlen, **kw)

    def score(self, inp_seq, tar_seq=None):
        """Teacher-forced scoring of any number of sequences (engine.score; the rule is in include/skf.h): how likely tar_seq is
        under the model that has encoded inp_seq.  tar_seq=None scores every sketch against itself (the autoencoding objective);
        otherwise row i of tar_seq - seq_len or seq_len + 1 columns, what predict / sample / beam_search return - is scored given
        row i of inp_seq.  A sequence counts through its EOS (the tokenizer's); see ``score_in_chunks`` for the chunking and the
        returned dict of host arrays: 'logp', 'length', 'token_logp', 'rank', 'perplexity', 'complete'.  A row's result depends
        neither on the number of rows, nor on its chunk, nor on its neighbours.  Token models only."""
        from .. import engine as _engine
        if self.dataset.hps['use_continuous_data']:
            raise ValueError(_engine.SCORING_NEEDS_TOKENS)
        if not self.hps['do_reconstruction']:
            raise ValueError("do_reconstruction is off")
        eos = self._sos_eos()[1]

        def score_chunk(inp, tar, m):
            return [t.cpu().numpy() for t in self.engine.score(inp, tar, n_valid=m, eos=eos)]
        return score_in_chunks(inp_seq, tar_seq, self.seq_len, self.engine.cfg.batch, eos, score_chunk)

    def load_reference_checkpoint(self, prefix):
        """Weights (+ Adam slots, optimizer.iterations, current_step) from a checkpoint written by the reference's
        tf.train.Checkpoint(transformer=..., optimizer=...) (core/models.py:321-344), read without TensorFlow."""
        import torch
        from ..utils import tf_checkpoint
        params, m, v, scalars = tf_checkpoint.load_reference_checkpoint(prefix, self.engine.entries)
        e = self.engine
        e.load_numpy(params)
        e.adam_m.zero_()
        e.adam_v.zero_()
        e.load_numpy(m, "adam_m")
        e.load_numpy(v, "adam_v")
        if 'iterations' in scalars:
            e.state[0] = int(scalars['iterations'])
        self.current_step = int(scalars.get('current_step', scalars.get('iterations', 0)))
        torch.cuda.synchronize()
        e.assert_replicas_equal()

    # ---- checkpoint payload
    def state_dict(self):
        e = self.engine
        e.synchronize()
        return {'params': e.params.cpu(), 'adam_m': e.adam_m.cpu(), 'adam_v': e.adam_v.cpu(), 'metrics': e.metrics.cpu(),
                'iterations': e.iterations, 'entries': e.entries}

    def prepare_metrics_for_save(self):
        self.engine.fold_metric_accumulators_into_rank0()

    def load_state_dict(self, state):
        e = self.engine
        e.params.copy_(state['params'])
        e.adam_m.copy_(state['adam_m'])
        e.adam_v.copy_(state['adam_v'])
        e.metrics.copy_(state['metrics'])
        if e.rank != 0:      # the file holds the accumulators of ALL ranks (folded into rank 0 before the save): one copy only
            e.zero_metric_accumulators()
        e.state[0] = int(state['iterations'])
        e.assert_replicas_equal()
