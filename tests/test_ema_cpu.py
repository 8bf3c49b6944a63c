"""CPU tests of weight averaging: the float32 reference against hand values, the host form of the decay against the reference bit
for bit, the rule of ``decay``, the new entries in the header and the binding table, and the new model in the registry."""
import os
import re

import numpy as np
import pytest

import ema_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skf_weight_average_validate", "skf_ema_decay_at", "skf_ema_update", "skf_buffer_swap", "skf_model_set_weight_average",
       "skf_model_update_weight_average", "skf_model_swap_weight_average", "skf_model_weight_average_live")
F = np.float32


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def test_reference_against_hand_values():
    assert ref.decay_at(0.999, True, 0) == F(0.1) and ref.decay_at(0.999, True, 0).dtype == F
    assert ref.decay_at(0.999, False, 0) == F(0.999) == ref.decay_at(0.999, False, 10 ** 9)
    assert ref.decay_at(0.999, True, 1) == F(2.0) / F(11.0)
    # (1 + n) / (10 + n) >= 0.999 from n = 8990 on (8991 / 9000 is 0.999): below it the ramp, from there the cap
    assert ref.decay_at(0.999, True, 8989) == F(8990.0) / F(8999.0) < F(0.999)
    for n in (8990, 8991, 10 ** 6, 2 ** 24 + 1, 2 ** 40):
        assert ref.decay_at(0.999, True, n) == F(0.999), n
    assert ref.decay_at(0.9, True, 79) == F(80.0) / F(89.0) < F(0.9) and ref.decay_at(0.9, True, 89) == F(0.9)
    # n is float32: 2^24 + 1 is not representable and becomes 2^24
    assert ref.decay_at(0.99999999, True, 2 ** 24 + 1) == ref.decay_at(0.99999999, True, 2 ** 24)
    # the update: 1 - (1 - 3) * 0.25 = 1.5; each operation rounded once
    out = ref.update([1.0, 3.0, 0.1], [3.0, 3.0, 0.3], 0.25)
    assert out.dtype == F and out[0] == F(1.5) and out[1] == F(3.0)
    assert out[2] == F(0.1) - (F(0.1) - F(0.3)) * F(0.25)
    assert np.isnan(ref.update([np.inf], [np.inf], 0.5))[0] and ref.update([1.0], [np.inf], 0.5)[0] == F(np.inf)
    assert ref.one_minus(ref.decay_at(0.999, True, 0)) == F(1.0) - F(0.1)


@pytest.mark.parametrize("decay", [0.999, 0.9, 0.5, 0.9999])
def test_host_decay_equals_the_reference_bit_for_bit(decay):
    from sketchformer_amd import build, ops
    build.build_library(verbose=False)
    for it in (0, 1, 89, 8990, 8991, 3000, 2 ** 24 + 1):
        for num_updates in (False, True):
            got = F(ops.ema_decay_at(decay, num_updates, it))
            assert _bits(got) == _bits(ref.decay_at(decay, num_updates, it)), (decay, num_updates, it, got)


def test_decay_rule_rejects_everything_outside_the_open_interval():
    from sketchformer_amd import build, engine
    build.build_library(verbose=False)
    for ok in (0.5, 0.999, 0.9999, np.float32(0.99), 1e-6):
        got = engine.check_weight_average(ok)
        assert type(got) is float and got == float(np.float32(ok))
    for bad in (0, 0.0, 1, 1.0, -0.5, -1, 2.0, float("inf"), float("-inf"), float("nan"), 1.0 - 1e-9, True, "0.9", None, [0.9]):
        with pytest.raises(ValueError, match="decay"):       # (1 - 1e-9 is 1.0 as a float32)
            engine.check_weight_average(bad)


def test_new_symbols_are_declared_and_bound():
    from sketchformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skf.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"int skf_ema_update\(float\* shadow, const float\* w, size_t n, float decay, int num_updates, const void\* step_state,\s*"
                     r"const void\* skip,\s*skf_stream_t stream\);", text)
    assert re.search(r"float skf_ema_decay_at\(float decay, int num_updates, long long iterations\);", text)
    assert re.search(r"int skf_buffer_swap\(float\* a, float\* b, size_t n, skf_stream_t stream\);", text)
    assert re.search(r"int skf_model_set_weight_average\(SkfModel\* m, float\* shadow, float decay, int num_updates\);", text)
    from sketchformer_amd import build
    assert "skf_ema.hip" in build.SOURCES and build.SOURCE_FLAGS["skf_ema.hip"] == ["-ffp-contract=off"]


def test_registry_finds_the_ema_model_and_its_hparams():
    from sketchformer_amd import models
    P = models.get_model_by_name("sketch-transformer-tf2")
    A = models.get_model_by_name("sketch-transformer-tf2-accum")
    M = models.get_model_by_name("sketch-transformer-tf2-ema")
    assert issubclass(M, A) and issubclass(M, P) and M.name == "sketch-transformer-tf2-ema"
    own = {"ema_decay": 0.0, "ema_num_updates": True, "ema_eval": True}
    assert M.specific_default_hparams().values() == {**A.specific_default_hparams().values(), **own}
    assert not set(own) & set(A.specific_default_hparams().values())
    assert M.quick_metrics == A.quick_metrics and M.slow_metrics == P.slow_metrics
    h = M.parse_hparams(base="batch_size=8", specific="ema_decay=0.999,ema_num_updates=false,accum_steps=2,global_clipnorm=0.5")
    assert (h.ema_decay, h.ema_num_updates, h.ema_eval, h.accum_steps, h.global_clipnorm) == (0.999, False, True, 2, 0.5)
    for Other in (P, A):
        with pytest.raises(ValueError):
            Other.parse_hparams(base=None, specific="ema_decay=0.9")
    # every public inference entry of the parent runs behind the lazy swap
    from sketchformer_amd.models import sketchformer_ema
    for name in ("encode_from_seq", "predict_class", "predict_from_embedding", "predict", "beam_search", "beam_search_from_embedding",
                 "interpolate", "sample", "sample_from_embedding", "complete", "complete_from_embedding", "score", "compute_metrics_from"):
        assert name in sketchformer_ema.AVERAGED_ENTRIES and getattr(M, name) is not getattr(A, name), name
