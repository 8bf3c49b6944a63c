"""Host side of beam search: the new symbols and their signatures, SkfBeam, every refusal of include/skf.h without a device, the
experiment's registration, and the invariants of the float64 restatement (tests/beam_reference.py) itself."""
import ctypes as C
import inspect

import numpy as np
import pytest

import beam_reference as ref


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def test_symbols_and_signatures(lib):
    from sketchformer_amd import _lib, engine, ops
    from sketchformer_amd.models.sketchformer import Transformer
    for name, nargs in (("skf_model_beam_decode", 13), ("skf_beam_advance", 17), ("skf_beam_finish", 15)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert list(inspect.signature(engine.TrainEngine.beam_decode).parameters) == [
        "self", "embedding", "expected_len", "n_valid", "sos", "eos", "max_steps", "beam_width", "length_alpha"]
    d = {k: v.default for k, v in inspect.signature(engine.TrainEngine.beam_decode).parameters.items()}
    assert d["beam_width"] == 4 and d["length_alpha"] == 0.0 and d["expected_len"] is None and d["n_valid"] is None
    assert list(inspect.signature(Transformer.beam_search).parameters) == ["self", "inp_seq", "beam_width", "length_alpha"]
    assert list(inspect.signature(Transformer.beam_search_from_embedding).parameters)[:4] == ["self", "emb", "beam_width", "length_alpha"]
    assert list(inspect.signature(ops.beam_step).parameters)[:7] == ["cand_logp", "cand_tok", "scores", "finished", "anc", "step", "eos"]
    assert _lib.BEAM_MAX == 8
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "skf.h")).read()
    assert "#define SKF_BEAM_MAX 8" in header


def test_beam_struct(lib):
    from sketchformer_amd import _lib
    assert C.sizeof(_lib.SkfBeam) == 12
    b = _lib.SkfBeam(beam_width=3, length_alpha=0.5)
    assert b.struct_size == 12 and [f[0] for f in _lib.SkfBeam._fields_] == ["struct_size", "beam_width", "length_alpha"]


def _create(lib, **kw):
    from sketchformer_amd import engine
    dims = dict(batch=4, seq_len=24, d_model=128, num_heads=2, dff=128, num_layers=2, vocab_size=52, n_classes=7, lowerdim=64,
                dropout_rate=0.0, use_graph=True)
    dims.update(kw)
    cfg = engine.make_config(**dims)
    m = C.c_void_p()
    assert lib.skf_model_create(C.byref(cfg), C.byref(m)) == 0, lib.skf_last_error()
    return m


def test_c_abi_refusals(lib):
    """every refusal is decided from the configuration and the arguments: the models here are created, never bound to a device"""
    from sketchformer_amd import _lib
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    el = (C.c_int * 4)(5, 5, 5, 5)

    def rc(m, W=2, alpha=0.0, n_valid=1, lens=None, size=None):
        bm = _lib.SkfBeam(beam_width=W, length_alpha=alpha)
        if size is not None:
            bm.struct_size = size
        return lib.skf_model_beam_decode(m, p, lens, n_valid, 50, 51, 4, p, p, p, None, C.byref(bm), None)

    m = _create(lib)
    for kw, word in ((dict(W=0), b"beam_width"), (dict(W=9), b"beam_width"), (dict(W=-1), b"beam_width"), (dict(W=8), b"beam_width"),
                     (dict(alpha=-0.5), b"length_alpha"), (dict(alpha=float("inf")), b"length_alpha"),
                     (dict(alpha=float("nan")), b"length_alpha"), (dict(size=8), b"struct_size"),
                     (dict(n_valid=3), b"n_valid"), (dict(n_valid=0), b"n_valid")):
        assert rc(m, **kw) == -1, kw                                   # W = 8 > batch = 4
        assert word in lib.skf_last_error(), (kw, lib.skf_last_error())
    assert rc(m) == -1 and b"not bound" in lib.skf_last_error()        # well-formed: only the missing device stands in the way
    assert rc(m, W=4, alpha=1.0) == -1 and b"not bound" in lib.skf_last_error()
    lib.skf_model_destroy(m)
    m = _create(lib, batch=8, vocab_size=4)                             # W <= vocab
    assert rc(m, W=5) == -1 and b"vocab_size" in lib.skf_last_error()
    lib.skf_model_destroy(m)
    m = _create(lib, continuous=True, vocab_size=None)
    assert rc(m) == -1 and b"continuous" in lib.skf_last_error()
    lib.skf_model_destroy(m)
    m = _create(lib, d_model=256, num_heads=2)                          # head size 128: not a model of the one-launch kernel
    assert rc(m) == -1 and b"one-launch" in lib.skf_last_error()
    lib.skf_model_destroy(m)
    m = _create(lib, blind_decoder_mask=False)
    assert rc(m) == -1 and b"expected_len" in lib.skf_last_error()
    assert rc(m, lens=el) == -1 and b"not bound" in lib.skf_last_error()
    lib.skf_model_destroy(m)
    assert lib.skf_model_beam_decode(None, p, None, 1, 0, 0, 1, p, p, p, None, None, None) == -1
    # the stand-alone merge checks its shapes before it launches
    adv = lambda n=1, W=2, step=0, ld=4: lib.skf_beam_advance(p, p, n, W, step, 1, p, p, p, p, ld, p, ld, p, ld, None, None)   # noqa: E731
    assert adv(W=0) == -1 and adv(W=9) == -1 and adv(n=0) == -1 and adv(step=-1) == -1 and adv(step=3) == -1
    fin = lambda n=1, W=2, ncols=3, T=4, alpha=0.0: lib.skf_beam_finish(p, p, p, 4, p, 4, n, W, ncols, T, alpha, p, p, p, None)   # noqa: E731
    assert fin(W=0) == -1 and fin(W=9) == -1 and fin(n=0) == -1 and fin(ncols=0) == -1 and fin(ncols=5, T=5) == -1
    assert fin(alpha=-1.0) == -1 and fin(alpha=float("nan")) == -1
    assert list(inspect.signature(__import__("sketchformer_amd.ops", fromlist=["ops"]).beam_finish).parameters)[:6] == [
        "scores", "lengths", "anc", "tokens", "beam_width", "length_alpha"]


class _Stub:
    """what Transformer.beam_search / beam_search_from_embedding read before they touch the engine"""

    def __init__(self, continuous, **hps):
        from sketchformer_amd.models.sketchformer import Transformer
        self.obj = Transformer.__new__(Transformer)
        self.obj.hps = dict(do_reconstruction=True, lowerdim=32, blind_decoder_mask=True, **hps)

        class _Data:
            pass
        self.obj.dataset = _Data()
        self.obj.dataset.hps = dict(use_continuous_data=continuous)


def test_python_refusals():
    from sketchformer_amd import engine
    emb = np.zeros((2, 32), np.float32)
    x = np.ones((2, 24), np.int64)
    tokens, cont = _Stub(False).obj, _Stub(True).obj
    for call in (lambda m, **kw: m.beam_search_from_embedding(emb, **kw), lambda m, **kw: m.beam_search(x, **kw)):
        with pytest.raises(ValueError, match="token models"):
            call(cont)
        for bad in (dict(beam_width=0), dict(beam_width=9), dict(beam_width=2.5), dict(length_alpha=-1.0),
                    dict(length_alpha=float("nan")), dict(length_alpha=float("inf"))):
            with pytest.raises(ValueError, match=list(bad)[0]):
                call(tokens, **bad)
    off = _Stub(False).obj
    off.hps['do_reconstruction'] = False
    with pytest.raises(ValueError, match="do_reconstruction"):
        off.beam_search(x)
    engine.check_beam(1, 0.0)
    engine.check_beam(8, 2.0, vocab_size=8, batch=8)
    with pytest.raises(ValueError, match="vocab_size"):
        engine.check_beam(4, 0.0, vocab_size=3, batch=8)
    with pytest.raises(ValueError, match="batch"):
        engine.check_beam(4, 0.0, vocab_size=30, batch=2)


def test_experiment_is_registered_with_its_defaults():
    from sketchformer_amd import experiments
    Exp = experiments.get_experiment_by_name('beam-reconstructions')
    assert Exp.requires_model is True
    want = dict(set_type='valid', n_sketches=8, beam_width=4, length_alpha=0.0, target_file='beam_reconstructions.npz')
    assert dict(Exp.specific_default_hparams().values()) == want


# ---------------------------------------------------------------- the restatement's own invariants
def _toy_model(V, seed):
    """a deterministic 'decoder': the logits of a prefix depend on its last two tokens and its length"""
    rng = np.random.RandomState(seed)
    A = rng.randn(V, V) * 1.5
    Bm = rng.randn(V, V) * 0.7
    t = rng.randn(64, V) * 0.3

    def fn(prefixes):
        prefixes = np.asarray(prefixes)
        prev = prefixes[:, -2] if prefixes.shape[1] > 1 else prefixes[:, -1]
        return A[prefixes[:, -1]] + Bm[prev] + t[prefixes.shape[1]]
    return fn


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_width_one_is_argmax_decoding(seed):
    V, sos, eos = 12, 10, 11
    fn = _toy_model(V, seed)
    got = ref.beam_search(fn, 1, sos, eos, 20)
    seq, score = [sos], 0.0
    for _ in range(20):
        lp = ref.log_softmax(fn(np.array([seq]))[0])
        tok = int(np.argmax(lp))                  # first index on ties, like the greedy kernel
        seq.append(tok)
        score += lp[tok]
        if tok == eos:
            break
    assert got["tokens"][0].tolist() == seq
    assert abs(got["scores"][0] - score) < 1e-12
    assert got["lengths"][0] == len(seq) - 1


@pytest.mark.parametrize("W", [2, 3, 4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_hypotheses_are_distinct_and_ranked(W, seed):
    V, sos, eos = 12, 10, 11
    got = ref.beam_search(_toy_model(V, seed), W, sos, eos, 16)
    rows = set()
    for r in range(W):
        n = got["lengths"][r] + 1
        assert np.isfinite(got["scores"][r])
        if got["finished"][r]:
            assert got["tokens"][r, n - 1] == eos and (got["tokens"][r, n:] == ref.PAD).all()
        rows.add(tuple(got["tokens"][r].tolist()))
    assert len(rows) == W                                           # distinct
    assert (np.diff(got["scores"]) <= 0).all()                      # non-increasing at alpha = 0


def test_finished_beam_offers_itself_once_and_ties_follow_parent_then_token():
    lp = np.log(np.array([[0.5, 0.3, 0.2], [0.5, 0.3, 0.2], [0.5, 0.3, 0.2]]))
    tk = np.array([[4, 2, 7], [4, 2, 7], [1, 2, 3]])
    # beams 0 and 1 tie exactly; beam 2 is finished and out-scores everything
    s, ranked = ref.merge(np.array([-1.0, -1.0, -0.1]), [0, 0, 1], [0, 0, 2], lp, tk, 5, eos=9)
    assert s["parent"].tolist() == [2, 0, 1] and s["token"].tolist() == [0, 4, 4]
    assert s["finished"].tolist() == [1, 0, 0] and s["length"].tolist() == [2, 6, 6]
    assert s["score"][0] == -0.1 and ref.margin(ranked, 3) == 0.0
    assert np.isinf(ranked[-2:]).all()                               # the finished beam's other two offers
    # all finished: every beam survives as itself, in score order
    s, _ = ref.merge(np.array([-3.0, -1.0, -2.0]), [1, 1, 1], [4, 2, 3], lp, tk, 7, eos=9)
    assert s["parent"].tolist() == [1, 2, 0] and s["token"].tolist() == [0, 0, 0] and s["length"].tolist() == [2, 3, 4]
    # length normalisation: a long lower sum overtakes a short higher one
    assert ref.final_order([-2.0, -2.4], [1, 9], 0.0).tolist() == [0, 1]
    assert ref.final_order([-2.0, -2.4], [1, 9], 1.0).tolist() == [1, 0]
    anc = np.array([[0, 1, 0], [1, 1, 0], [2, 0, 0]])
    assert ref.next_ancestry(anc, [2, 0, 1], 1, base=6).tolist() == [[2, 0, 6], [0, 1, 7], [1, 1, 8]]
