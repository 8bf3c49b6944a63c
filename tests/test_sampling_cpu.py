"""Host side of the sampled decode: the counter-based uniform stream, the selection rule of tests/sampling_reference.py on
hand-made rows, the argument checks of every layer and the experiment's registration (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import sampling_reference as ref


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def _draws(lib, seed, streams, steps):
    return np.array([[lib.skf_sample_uniform(seed, s, t) for t in steps] for s in streams], dtype=np.float64)


def test_uniform_stream(lib):
    u = _draws(lib, 7, range(500), range(200))                            # 10^5 draws over (stream, step)
    assert (u >= 0).all() and (u < 1).all()
    n = u * 2.0 ** 24
    assert np.array_equal(n, np.round(n))                                 # multiples of 2^-24
    assert np.array_equal(u, _draws(lib, 7, range(500), range(200)))      # a pure function of its three arguments
    # 64 equal bins: chi-square has mean 63 and variance 126
    counts = np.bincount((u.reshape(-1) * 64).astype(np.int64), minlength=64)
    expect = u.size / 64.0
    chi2 = ((counts - expect) ** 2 / expect).sum()
    assert abs(chi2 - 63.0) <= 5.0 * np.sqrt(126.0), chi2
    # along a stream as well as across streams
    for axis in (0, 1):
        assert abs(u.mean(axis=axis) - 0.5).max() <= 5.0 * np.sqrt(1.0 / 12.0 / u.shape[axis])
    # changing any one of seed / stream / step changes the sequence
    base = _draws(lib, 7, [3], range(64))[0]
    assert not np.array_equal(base, _draws(lib, 8, [3], range(64))[0])
    assert not np.array_equal(base, _draws(lib, 7, [4], range(64))[0])
    assert not np.array_equal(base, _draws(lib, 7, [3], range(1, 65))[0])
    assert np.array_equal(base[1:], _draws(lib, 7, [3], range(1, 64))[0])
    from sketchformer_amd import ops
    assert ops.sample_uniform(7, 3, 5) == base[5]


def test_rule_top_k_keeps_ties_at_the_threshold():
    row = np.array([0.0, 2.0, 1.0, 1.0, -1.0, 1.0, 3.0])
    keep, e = ref.survivors(row, (1.0, 3, 1.0))                           # third largest = 1.0, held three times
    assert keep.tolist() == [False, True, True, True, False, True, True]
    assert (e[~keep] == 0).all() and np.allclose(e[keep], np.exp(row[keep] - 3.0))
    assert not ref.ambiguous(row, (1.0, 3, 1.0))                          # equal values share one fate: nothing to perturb
    assert ref.ambiguous(np.array([0.0, 2.0, 1.0, 1.0 - 5e-5, 3.0]), (1.0, 3, 1.0))
    assert not ref.ambiguous(np.array([0.0, 2.0, 1.0, 1.0 - 5e-4, 3.0]), (1.0, 3, 1.0))
    # the temperature scales the gap
    assert ref.ambiguous(np.array([0.0, 2.0, 1.0, 1.0 - 5e-4, 3.0]), (10.0, 3, 1.0))


def test_rule_cuts_that_are_off():
    row = np.array([0.5, -0.25, 2.0, 1.0])
    p = np.exp(row - 2.0) / np.exp(row - 2.0).sum()
    for params in ((1.0, 0, 1.0), (1.0, 4, 1.0), (1.0, 9, 1.0)):          # top_k = 0, = V, > V; top_p = 1
        keep, e = ref.survivors(row, params)
        assert keep.all() and np.allclose(e / e.sum(), p)
        assert not ref.ambiguous(row, params)
    # the draw is the inverse CDF in index order
    c = np.cumsum(p)
    for u in (0.0, c[0] - 1e-9, c[0] + 1e-9, c[1] + 1e-9, c[2] + 1e-9, 1 - 2.0 ** -24):
        want = int(np.searchsorted(c, u, side="right"))
        assert ref.sample(row, (1.0, 0, 1.0), u) == want
        assert ref.accepts(row, (1.0, 0, 1.0), u, want)
    assert not ref.accepts(row, (1.0, 0, 1.0), 0.0, 2)
    assert ref.accepts(row, (1.0, 0, 1.0), c[0] + 5e-5, 0) and not ref.accepts(row, (1.0, 0, 1.0), c[0] + 5e-4, 0)
    # temperature: z = logits / T
    keep, e = ref.survivors(row, (0.5, 0, 1.0))
    assert np.allclose(e, np.exp(2 * (row - 2.0)))


def test_rule_nucleus():
    row = np.log(np.array([0.1, 0.4, 0.2, 0.2, 0.1]))
    # mass above: 0.4 -> 0, the two 0.2 -> 0.4, the two 0.1 -> 0.8
    assert ref.survivors(row, (1.0, 0, 0.85))[0].tolist() == [True] * 5
    assert ref.survivors(row, (1.0, 0, 0.75))[0].tolist() == [False, True, True, True, False]      # ties share one fate
    assert ref.survivors(row, (1.0, 0, 0.45))[0].tolist() == [False, True, True, True, False]
    assert ref.survivors(row, (1.0, 0, 0.35))[0].tolist() == [False, True, False, False, False]
    assert ref.survivors(row, (1.0, 0, 1e-6))[0].tolist() == [False, True, False, False, False]    # tiny: only the maximum
    assert not ref.ambiguous(row, (1.0, 0, 1e-6))
    assert ref.ambiguous(row, (1.0, 0, 0.8 + 5e-5)) and not ref.ambiguous(row, (1.0, 0, 0.75))
    for u in (0.0, 0.3, 0.999):
        assert ref.sample(row, (1.0, 0, 1e-6), u) == 1
    # over what top-k kept: top_k = 3 keeps {0.4, 0.2, 0.2}, S = 0.8; the 0.2s have 0.4 above them
    assert ref.survivors(row, (1.0, 3, 0.55))[0].tolist() == [False, True, True, True, False]
    assert ref.survivors(row, (1.0, 3, 0.45))[0].tolist() == [False, True, False, False, False]
    # survivors in index order: u just past the first survivor's share lands on the next survivor, not on a dropped entry
    assert ref.sample(row, (1.0, 0, 0.75), 0.5 + 1e-9) == 2 and ref.sample(row, (1.0, 0, 0.75), 0.75 + 1e-9) == 3


def test_rule_one_entry_row_and_minus_infinity():
    for params in ((1.0, 0, 1.0), (0.3, 1, 0.5), (2.0, 5, 1e-3)):
        assert ref.survivors(np.array([-4.0]), params)[0].tolist() == [True]
        assert ref.sample(np.array([-4.0]), params, 0.999) == 0 and ref.accepts(np.array([-4.0]), params, 0.5, 0)
    row = np.array([-np.inf, 0.0, -np.inf, 0.0])
    keep, e = ref.survivors(row, (1.0, 3, 1.0))
    assert keep.all() and e.tolist() == [0.0, 1.0, 0.0, 1.0]              # the third largest is -inf: a tie, kept, without mass
    assert ref.sample(row, (1.0, 3, 1.0), 0.25) == 1 and ref.sample(row, (1.0, 3, 1.0), 0.75) == 3
    assert not ref.ambiguous(row, (1.0, 3, 1.0)) and not ref.accepts(row, (1.0, 3, 1.0), 0.25, 3)


class _Stub:
    """what Transformer.sample / sample_from_embedding read before they touch the engine"""

    def __init__(self, continuous, **hps):
        from sketchformer_amd.models.sketchformer import Transformer
        self.obj = Transformer.__new__(Transformer)
        self.obj.hps = dict(do_reconstruction=True, lowerdim=32, blind_decoder_mask=True, **hps)

        class _Data:
            pass
        self.obj.dataset = _Data()
        self.obj.dataset.hps = dict(use_continuous_data=continuous)


def test_model_level_argument_errors(lib):
    from sketchformer_amd import _lib, engine
    emb = np.zeros((2, 32), np.float32)
    x = np.ones((2, 24), np.int64)
    tokens, cont = _Stub(False).obj, _Stub(True).obj
    for call in (lambda m, **kw: m.sample_from_embedding(emb, **kw), lambda m, **kw: m.sample(x, **kw)):
        with pytest.raises(ValueError, match="token models"):
            call(cont)
        for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-1), dict(top_k=2.5),
                    dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):
            with pytest.raises(ValueError, match=list(bad)[0]):
                call(tokens, **bad)
    with pytest.raises(ValueError, match="n_samples"):
        tokens.sample_from_embedding(emb, n_samples=0)
    engine.check_sampling(0.7, 40, 0.9)
    engine.check_sampling(1.0, 0, 1.0)
    # the C ABI answers the same way before any launch (the pointers are never read)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)

    def rc(**kw):
        smp = _lib.SkfSampling(**dict(dict(temperature=1.0, top_k=0, top_p=1.0, seed=0), **kw))
        return lib.skf_decode_sample_tokens(p, 4, 1, 4, 1, 0, -1, p, 2, p, 2, p, p, None, None, C.byref(smp), p, None)
    for bad in (dict(temperature=0.0), dict(temperature=-2.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.0001)):
        assert rc(**bad) == -1, bad
        assert list(bad)[0].encode() in lib.skf_last_error()
    assert rc(struct_size=16) == -1 and b"struct_size" in lib.skf_last_error()
    assert C.sizeof(_lib.SkfSampling) == 20
    assert lib.skf_model_sample_decode(None, None, None, 1, 0, 0, 1, p, None, None, None, None) == -1


def test_experiment_is_registered_with_its_defaults():
    from sketchformer_amd import experiments
    Exp = experiments.get_experiment_by_name('sampled-reconstructions')
    assert Exp.requires_model is True
    want = dict(set_type='valid', n_sketches=8, n_samples=6, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                target_file='sampled_reconstructions.npz', plot_file='sampled_reconstructions.png')
    assert dict(Exp.specific_default_hparams().values()) == want


def test_bf16_plan_keeps_its_decode_areas_apart(lib):
    """skf_model_create checks that every decode area of the bf16 plan is an allocation of its own (the stream ids share
    dc_limit's; an area left unallocated would sit at offset 0, on the staged input): a bf16 model is created without a device"""
    from sketchformer_amd import engine
    cfg = engine.make_config(batch=4, seq_len=24, d_model=128, num_heads=2, dff=128, num_layers=2, vocab_size=52, n_classes=7,
                             lowerdim=64, dropout_rate=0.0, use_graph=True, act_dtype="bf16")
    m = C.c_void_p()
    assert lib.skf_model_create(C.byref(cfg), C.byref(m)) == 0, lib.skf_last_error()
    lib.skf_model_destroy(m)


def test_fp32_plan_keeps_its_decode_areas_apart(lib):
    """The same check runs on the fp32 plan, whose decode areas come from the same allocation (its stream ids, too, are the second
    half of the key-limit area): an fp32 model that captures its step creates no stream or event, so it is created without a device"""
    from sketchformer_amd import engine
    cfg = engine.make_config(batch=4, seq_len=24, d_model=128, num_heads=2, dff=128, num_layers=2, vocab_size=52, n_classes=7,
                             lowerdim=64, dropout_rate=0.0, use_graph=True)
    m = C.c_void_p()
    assert lib.skf_model_create(C.byref(cfg), C.byref(m)) == 0, lib.skf_last_error()
    lib.skf_model_destroy(m)
