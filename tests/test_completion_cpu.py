"""Host side of sketch completion (include/skf.h: prefix-forced decoding): the new symbols and SkfPrefix, what engine.check_prefix
accepts and rejects, the refusals the C entries decide without a device, the experiment's cut and aggregation on hand-made rows,
and the float64 restatement (tests/completion_reference.py) itself."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import completion_reference as ref


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def test_symbols_struct_and_keywords(lib):
    from sketchformer_amd import _lib, engine
    from sketchformer_amd.models.sketchformer import Transformer
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "skf.h")).read()
    for name, nargs in (("skf_model_prefix_decode", 13), ("skf_model_beam_prefix_decode", 14)):
        assert "int %s(" % name in header
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert "typedef struct SkfPrefix {" in header
    assert [f[0] for f in _lib.SkfPrefix._fields_] == ["struct_size", "tokens", "ld", "len_host", "stepwise"]
    assert C.sizeof(_lib.SkfPrefix) == 40 and _lib.SkfPrefix().struct_size == 40
    for fn in (engine.TrainEngine.greedy_decode, engine.TrainEngine.sample_decode):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items()}
        assert d["prefix"] is None and d["prefix_len"] is None and d["prefill"] is True
    # beam search behind a prefix is a method of its own: beam_decode's parameter list is pinned by tests/test_beam_cpu.py
    assert list(inspect.signature(engine.TrainEngine.beam_complete).parameters) == [
        "self", "embedding", "prefix", "prefix_len", "expected_len", "n_valid", "sos", "eos", "max_steps", "beam_width", "length_alpha"]
    assert list(inspect.signature(Transformer.complete_from_embedding).parameters) == [
        "self", "emb", "prefix", "prefix_len", "expected_len", "mode", "n_samples", "temperature", "top_k", "top_p", "seed",
        "beam_width", "length_alpha", "prefill"]
    assert list(inspect.signature(Transformer.complete).parameters)[:2] == ["self", "partial_seq"]


def test_check_prefix_lengths_and_padding_rows():
    from sketchformer_amd.engine import check_prefix
    p = np.array([[5, 6, 7, 8], [9, 10, 11, 12]])
    tok, lens = check_prefix(p, [3, 0], rows=4, max_steps=24, vocab_size=52)
    assert tok.dtype == np.int64 and tok.shape == (4, 4) and lens.dtype == np.int32
    assert lens.tolist() == [3, 0, 3, 3]                          # rows beyond the caller's copy row 0: the shortest prefix stays
    assert np.array_equal(tok[:2], p) and np.array_equal(tok[2], p[0]) and np.array_equal(tok[3], p[0])
    assert check_prefix(p, [4, 4], 2, 4, 52)[1].tolist() == [4, 4]          # len == max_steps == the width
    with pytest.raises(ValueError, match="max_steps"):
        check_prefix(p, [4, 4], 2, 3, 52)
    with pytest.raises(ValueError, match="max_steps"):
        check_prefix(p, [-1, 2], 2, 24, 52)
    with pytest.raises(ValueError, match="columns"):
        check_prefix(p, [5, 2], 2, 24, 52)                        # longer than the prefix given
    with pytest.raises(ValueError, match="one length per"):
        check_prefix(p, [1], 2, 24, 52)
    with pytest.raises(ValueError, match="rows"):
        check_prefix(p, [1, 1], 1, 24, 52)                        # more prefixes than rows
    with pytest.raises(ValueError):
        check_prefix(np.zeros((2, 3), np.float32), [1, 1], 2, 24, 52)
    tok, lens = check_prefix(np.zeros((1, 0), np.int64), [0], 2, 24, 52)     # nothing to force: ld is still a valid pitch
    assert tok.shape == (2, 1) and lens.tolist() == [0, 0]


def test_check_prefix_token_range():
    from sketchformer_amd.engine import check_prefix
    p = np.array([[5, 52, 7], [1, 2, -3]])
    with pytest.raises(ValueError, match="out of range"):
        check_prefix(p, [3, 1], 2, 24, 52)
    with pytest.raises(ValueError, match="out of range"):
        check_prefix(p, [1, 3], 2, 24, 52)
    tok, lens = check_prefix(p, [1, 2], 2, 24, 52)                # out-of-range tokens behind the lengths are never forced
    assert lens.tolist() == [1, 2]


def test_check_prefix_derives_lengths_at_the_first_eos_or_pad():
    from sketchformer_amd.engine import check_prefix
    eos = 51
    p = np.array([[5, 6, eos, 8, 0],          # EOS first
                  [5, 0, 7, eos, 9],          # PAD first
                  [eos, 1, 2, 3, 4],          # nothing in front of the EOS
                  [1, 2, 3, 4, 5]])           # neither: the whole row
    tok, lens = check_prefix(p, None, 4, 24, 52, eos=eos)
    assert lens.tolist() == [2, 1, 0, 5]
    with pytest.raises(ValueError, match="max_steps"):
        check_prefix(p, None, 4, 4, 52, eos=eos)                  # the derived length of row 3 is 5


def test_c_entries_refuse_without_a_device(lib):
    """decided from the configuration and the arguments: the models here are created, never bound"""
    from sketchformer_amd import _lib, engine
    assert lib.skf_model_prefix_decode(None, None, None, 1, 0, 0, 1, None, None, None, None, None, None) == -1
    assert lib.skf_model_beam_prefix_decode(None, None, None, 1, 0, 0, 1, None, None, None, None, None, None, None) == -1
    cfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=32,
                             dropout_rate=0.0, use_graph=True)       # (no side stream: nothing here needs a device)
    m = C.c_void_p()
    assert lib.skf_model_create(C.byref(cfg), C.byref(m)) == 0, lib.skf_last_error()
    try:
        buf = (C.c_char * 64)()
        p = C.cast(buf, C.c_void_p)
        bm = _lib.SkfBeam(beam_width=2, length_alpha=0.0)
        el = (C.c_int * 4)(5, 5, 5, 5)
        # a null prefix is refused by both entries before anything else
        assert lib.skf_model_prefix_decode(m, p, None, 4, 50, 51, 8, p, None, None, None, None, None) == -1
        assert b"SkfPrefix" in lib.skf_last_error()
        assert lib.skf_model_beam_prefix_decode(m, p, el, 2, 50, 51, 8, p, p, p, None, C.byref(bm), None, None) == -1
        assert b"SkfPrefix" in lib.skf_last_error()

        def both(lens, max_steps=8, **kw):
            """[(return code, error text)] of the greedy entry (4 prefixes) and of the beam entry (2) on an SkfPrefix over `lens`"""
            arr = (C.c_int * 4)(*lens)
            pf = _lib.SkfPrefix(**dict(dict(tokens=C.cast(buf, C.c_void_p).value, ld=6, len_host=arr, stepwise=0), **kw))
            res = []
            for call in (lambda: lib.skf_model_prefix_decode(m, p, None, 4, 50, 51, max_steps, p, None, C.byref(pf), None, None, None),
                         lambda: lib.skf_model_beam_prefix_decode(m, p, el, 2, 50, 51, max_steps, p, p, p, None, C.byref(bm), C.byref(pf),
                                                                  None)):
                rc = call()
                res.append((rc, lib.skf_last_error()))
            return res
        for lens, kw, what in (([1, 2, 3, 4], dict(struct_size=36), b"struct_size"),
                               ([1, 7, 3, 4], {}, b"ld must not be smaller"),              # ld = 6
                               ([9, 2, 3, 4], dict(ld=16), b"[0, max_steps]"),             # max_steps = 8
                               ([-1, 2, 3, 4], {}, b"[0, max_steps]"),
                               ([1, 2, 3, 4], dict(tokens=None), b"null prefix tokens"),
                               ([1, 2, 3, 4], dict(max_steps=25), b"max_steps must be in [1, seq_len]")):
            for rc, err in both(lens, **kw):
                assert rc == -1 and what in err, (lens, kw, rc, err)
        # a good prefix passes every check that needs no device: what is left to refuse is that the model is not bound
        for rc, err in both([0, 6, 3, 8], ld=8):
            assert rc == -1 and b"model not bound" in err, (rc, err)
        # the beam entry reads one length per sketch (batch / beam_width = 2): the third length is none of its business
        (rc_g, err_g), (rc_b, err_b) = both([1, 2, 99, 4])
        assert rc_g == -1 and b"[0, max_steps]" in err_g and rc_b == -1 and b"model not bound" in err_b
    finally:
        lib.skf_model_destroy(m)
    # a continuous model: SKF_EUNSUPPORTED from the greedy / sampled entry (the beam entry refuses such a model as it always did)
    ccfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=None, n_classes=7, lowerdim=32,
                              dropout_rate=0.0, use_graph=True, continuous=True)
    cm = C.c_void_p()
    assert lib.skf_model_create(C.byref(ccfg), C.byref(cm)) == 0, lib.skf_last_error()
    try:
        arr = (C.c_int * 4)(1, 2, 3, 4)
        pf = _lib.SkfPrefix(tokens=C.cast(buf, C.c_void_p).value, ld=6, len_host=arr, stepwise=0)
        assert lib.skf_model_prefix_decode(cm, p, None, 4, 0, 0, 8, p, None, C.byref(pf), None, None, None) == -2
        assert b"continuous" in lib.skf_last_error()
    finally:
        lib.skf_model_destroy(cm)


# ---------------------------------------------------------------- the experiment's plain functions
def test_cut_sketches():
    from sketchformer_amd.experiments.sketch_completion import cut_sketches
    sos, eos = 50, 51
    x = np.array([[sos, 1, 2, 3, 4, eos, 0, 0],
                  [sos, 1, 2, 3, 4, 5, 6, 7],          # truncated: no EOS
                  [sos, eos, 0, 0, 0, 0, 0, 0],        # an empty sketch
                  [1, 2, 3, eos, 0, 0, 0, 0]])         # no start symbol
    part, kept, body = cut_sketches(x, 0.5, sos, eos)
    assert body.tolist() == [4, 7, 0, 3] and kept.tolist() == [2, 4, 0, 2]
    assert part.tolist() == [[sos, 1, 2, eos, 0, 0, 0, 0], [sos, 1, 2, 3, 4, eos, 0, 0], [sos, eos, 0, 0, 0, 0, 0, 0],
                             [1, 2, eos, 0, 0, 0, 0, 0]]
    part, kept, _ = cut_sketches(x, 0.0, sos, eos)
    assert kept.tolist() == [0, 0, 0, 0]
    assert part[:, :2].tolist() == [[sos, eos], [sos, eos], [sos, eos], [eos, 0]] and (part[:, 2:] == 0).all()
    part, kept, _ = cut_sketches(x, 1.0, sos, eos)
    assert kept.tolist() == [4, 7, 0, 3]
    assert np.array_equal(part, x)                     # the rows themselves; the truncated one has no room for an EOS
    assert part.dtype == x.dtype
    with pytest.raises(ValueError):
        cut_sketches(x, 1.5, sos, eos)
    with pytest.raises(ValueError):
        cut_sketches(x[0], 0.5, sos, eos)


def test_aggregate():
    from sketchformer_amd.experiments.sketch_completion import aggregate, format_table
    ter = np.array([[0.5, 0.25, 0.75, 0.5], [0.0, 0.25, 0.25, 0.5]])
    dtw = np.array([[1.0, 2.0, 3.0, 2.0], [0.5, 0.5, 1.5, 1.5]])
    labels = np.array([3, 1, 4, 1])
    cp = np.array([[3, 1, 0, 0], [3, 1, 4, 0]])
    cc = np.array([[0, 0, 0, 0], [3, 1, 4, 1]])
    t = aggregate([0.25, 0.75], ter, dtw, labels, cp, cc)
    assert sorted(t) == ["class_accuracy_completed", "class_accuracy_partial", "dtw", "fraction", "token_error_rate"]
    assert t["fraction"].tolist() == [0.25, 0.75]
    assert t["token_error_rate"].tolist() == [0.5, 0.25] and t["dtw"].tolist() == [2.0, 1.0]
    assert t["class_accuracy_partial"].tolist() == [0.5, 0.75] and t["class_accuracy_completed"].tolist() == [0.0, 1.0]
    no_cls = aggregate([0.25, 0.75], ter, dtw, labels)
    assert np.isnan(no_cls["class_accuracy_partial"]).all() and np.isnan(no_cls["class_accuracy_completed"]).all()
    assert len(format_table(t).splitlines()) == 3
    with pytest.raises(ValueError):
        aggregate([0.25], ter, dtw, labels)


def test_experiment_is_registered():
    from sketchformer_amd import experiments
    Exp = experiments.get_experiment_by_name("sketch-completion")
    h = Exp.specific_default_hparams()
    assert h.fractions == [0.25, 0.5, 0.75] and h.source == "partial" and h.target_file == "sketch_completion.npz"
    assert Exp.parse_hparams("n_sketches=8,fractions=[0.5],source=full").fractions == [0.5]


# ---------------------------------------------------------------- the restatement itself
def test_reference_forces_and_stops():
    V, sos, eos = 10, 8, 9
    calls = []

    def fn(tokens):                                    # free positions: token = (last token + 1) mod 8, never EOS
        calls.append(tokens.shape[1] - 1)
        out = np.zeros((tokens.shape[0], V))
        out[np.arange(tokens.shape[0]), (tokens[:, -1] + 1) % 8] = 1.0
        return out
    prefix = np.array([[3, 99, eos, 1], [eos, 0, 0, 0]])
    tok, forced = ref.forced_greedy(fn, prefix, [3, 1], sos, eos, 6, V)
    assert tok.tolist() == [[sos, 3, 0, eos], [sos, eos, 2, 3]]          # 99 is out of range: PAD; the decode ends inside row 0's prefix
    assert forced.tolist() == [[False, True, True, True], [False, True, False, False]]
    assert calls == [1, 2]                             # no logits where every row is forced
    tok, forced = ref.forced_greedy(fn, prefix, [0, 0], sos, eos, 3, V)
    assert tok.tolist() == [[sos, 1, 2, 3], [sos, 1, 2, 3]] and not forced.any()
    tok, _ = ref.forced_greedy(fn, prefix, [3, 1], sos, eos, 6, V, n_valid=1)
    assert tok.shape[1] == 4
    tok, _ = ref.forced_greedy(fn, prefix, [1, 1], sos, eos, 5, V)         # row 0 never ends: max_steps positions
    assert tok.shape[1] == 6 and tok[0].tolist() == [sos, 3, 4, 5, 6, 7]
