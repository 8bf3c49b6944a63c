"""CPU tests of gradient accumulation: the rule of ``accum_steps``, the new entries in the header and the binding table, the host
form of the dropout key, and the new model in the registry."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skf_grad_accumulate", "skf_model_accumulate_gradients", "skf_step_drop_key")


def test_accum_steps_rule_accepts_counts_and_refuses_everything_else():
    from sketchformer_amd import engine
    for ok in (1, 2, 3, 64, engine.ACCUM_STEPS_MAX, np.int64(4), np.int32(1)):
        got = engine.check_gradient_accumulation(ok)
        assert got == int(ok) and type(got) is int
    for bad in (0, -1, engine.ACCUM_STEPS_MAX + 1, True, False, np.bool_(True), 2.0, 2.5, np.float32(2), "2", None, [2]):
        with pytest.raises(ValueError, match="accum_steps"):
            engine.check_gradient_accumulation(bad)
    assert engine.ACCUM_STEPS_MAX == 1024


def test_new_symbols_are_declared_and_bound():
    from sketchformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skf.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int skf_grad_accumulate\(float\* dst, const float\* a, const float\* b, size_t n, void\* step_state, int micro_op,\s*"
                     r"skf_stream_t stream\);", text)
    assert re.search(r"int skf_model_accumulate_gradients\(SkfModel\* m, float\* acc, int phase, skf_stream_t stream\);", text)
    consts = dict(re.findall(r"#define (SKF_(?:MICRO|ACCUM)_[A-Z]+) (\d+)", text))
    assert consts == {"SKF_MICRO_KEEP": "0", "SKF_MICRO_NEXT": "1", "SKF_MICRO_ZERO": "2",
                      "SKF_ACCUM_FIRST": "0", "SKF_ACCUM_ADD": "1", "SKF_ACCUM_CLOSE": "2", "SKF_ACCUM_RESET": "3"}
    assert (_lib.MICRO_KEEP, _lib.MICRO_NEXT, _lib.MICRO_ZERO) == (0, 1, 2)
    assert (_lib.ACCUM_FIRST, _lib.ACCUM_ADD, _lib.ACCUM_CLOSE, _lib.ACCUM_RESET) == (0, 1, 2, 3)
    # the spare word of the step state has its name, and the struct kept its size
    common = open(os.path.join(ROOT, "sketchformer_amd", "csrc", "skf_common.h")).read()
    body = re.search(r"struct SkfStepState \{(.*?)\n\};", common, flags=re.S).group(1)
    assert re.search(r"uint32_t micro;", body) and not re.search(r"\bpad\b", body)


def _hash32(x):
    x &= 0xffffffff
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def test_dropout_key_is_unchanged_at_micro_zero_and_never_a_shifted_iteration():
    """micro == 0: the two-round hash(seed, iterations) every step had (restated here).  micro = j > 0: a third round over j, and in
    particular not the key of iteration it + j nor of any (later iteration, micro) pair nearby."""
    from sketchformer_amd import build, ops
    build.build_library(verbose=False)
    old = lambda seed, it: _hash32(seed ^ _hash32((it + 0x632be5ab) & 0xffffffff))      # noqa: E731
    for seed in (0, 5, 1234, 0xdeadbeef):
        for it in (0, 1, 3000, 2 ** 31 - 1, 2 ** 32 + 7):
            assert ops.step_drop_key(seed, it, 0) == old(seed, it)
    seed, seen = 5, {}
    for it in range(3000, 3040):
        for j in range(0, 9):
            key = ops.step_drop_key(seed, it, j)
            assert key not in seen, ((it, j), seen.get(key))
            seen[key] = (it, j)
    for j in range(1, 9):
        assert ops.step_drop_key(seed, 3000, j) == _hash32(old(seed, 3000) ^ _hash32(j + 0x5bd1e995))
        assert ops.step_drop_key(seed, 3000, j) != old(seed, 3000 + j)


def test_registry_finds_the_accum_model_and_its_hparams():
    from sketchformer_amd import models
    P = models.get_model_by_name("sketch-transformer-tf2")
    Cl = models.get_model_by_name("sketch-transformer-tf2-clip")
    M = models.get_model_by_name("sketch-transformer-tf2-accum")
    assert issubclass(M, Cl) and issubclass(M, P) and M.name == "sketch-transformer-tf2-accum"
    assert M.specific_default_hparams().values() == {**Cl.specific_default_hparams().values(), "accum_steps": 1}
    assert "accum_steps" not in Cl.specific_default_hparams().values() and "accum_steps" not in P.specific_default_hparams().values()
    assert M.quick_metrics == Cl.quick_metrics and M.slow_metrics == P.slow_metrics
    h = M.parse_hparams(base="batch_size=8", specific="accum_steps=4,global_clipnorm=0.5")
    assert (h.accum_steps, h.global_clipnorm, h.batch_size) == (4, 0.5, 8)
    for Other in (P, Cl):
        with pytest.raises(ValueError):
            Other.parse_hparams(base=None, specific="accum_steps=4")
