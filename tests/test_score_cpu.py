"""Teacher-forced scoring without a device: the float64 restatement of the rule (tests/score_reference.py) against hand-worked
rows and against the oracle's reconstruction loss, and the host side of Transformer.score (chunking, the seq_len + 1 -> seq_len
window, `complete`, `perplexity`) driven by the restatement instead of the engine."""
import math

import numpy as np
import pytest

import oracle
import score_reference as ref

EOS = 7


# ---------------------------------------------------------------- 1. hand-worked rows
def test_scored_length_by_hand():
    assert ref.scored_length([3, 4, EOS, 0, 0], EOS) == 3              # through the EOS
    assert ref.scored_length([EOS, 3, 4, 0], EOS) == 1                 # EOS at position 0: it alone is scored
    assert ref.scored_length([3, 0, 4, EOS, 0], EOS) == 4              # a PAD in front of the EOS does not end the sequence
    assert ref.scored_length([3, 4, 0, 0, 5], EOS) == 2                # PAD without EOS: up to the first PAD
    assert ref.scored_length([0, 3, 4], EOS) == 0
    assert ref.scored_length([3, 4, 5, 6], EOS) == 4                   # no terminator
    assert ref.scored_length([3, 4, EOS, 5, EOS], EOS) == 3            # the FIRST EOS
    assert ref.scored_length([2, 0, 0], 0) == 2                        # a tokenizer without symbols: eos == PAD, and it is scored


def test_token_score_by_hand():
    ln = math.log
    # uniform row: log p = -ln V, ties at the lower indices only
    lp, rk = ref.token_score([1.0, 1.0, 1.0, 1.0], 2)
    assert lp == pytest.approx(-ln(4), abs=1e-15) and rk == 2
    # z = ln(1, 2, 3, 4): p = (.1, .2, .3, .4)
    z = np.log([1.0, 2.0, 3.0, 4.0])
    for y, p, r in ((0, .1, 3), (1, .2, 2), (2, .3, 1), (3, .4, 0)):
        lp, rk = ref.token_score(z, y)
        assert lp == pytest.approx(ln(p), abs=1e-14) and rk == r
    # the target's value duplicated at a lower AND at a higher index: only the lower one is ahead
    z = [0.5, 2.0, 0.5, 0.5, -1.0]
    assert ref.token_score(z, 2)[1] == 2                               # index 1 is larger, index 0 ties in front
    assert ref.token_score(z, 0)[1] == 1 and ref.token_score(z, 3)[1] == 3
    assert ref.token_score(z, 1)[1] == 0                               # rank 0 = the first-index argmax
    assert ref.token_score([2.0, 2.0], 0)[1] == 0 and ref.token_score([2.0, 2.0], 1)[1] == 1
    # magnitudes: a shift of the whole row changes nothing
    z = np.array([0.3, -1.2, 2.2, 0.0])
    for shift in (80.0, -80.0, 700.0):
        assert ref.token_score(z + shift, 1)[0] == pytest.approx(ref.token_score(z, 1)[0], abs=1e-12)
    # out of range: never an index
    assert ref.token_score(z, -1) == (-np.inf, 4) and ref.token_score(z, 4) == (-np.inf, 4)
    # -inf entries: a -inf target scores -inf (no NaN), the others add nothing
    zi = np.array([0.0, -np.inf, ln(3.0), -np.inf])
    lp, rk = ref.token_score(zi, 1)
    assert lp == -np.inf and rk == 2
    assert ref.token_score(zi, 3) == (-np.inf, 3)                      # the -inf at index 1 ties in front
    lp, rk = ref.token_score(zi, 0)
    assert lp == pytest.approx(-ln(4.0), abs=1e-15) and rk == 1


def test_sequence_score_by_hand():
    V, T = 4, 5
    z = np.tile(np.log([1.0, 2.0, 3.0, 4.0]), (3, T, 1))
    tar = np.array([[1, 2, 3, 0, 0],                                   # eos = 3 at t = 2
                    [1, 2, 0, 0, 1],                                   # PAD without EOS
                    [1, 2, 2, 1, 2]])                                  # neither
    z[0, 3:] = np.nan                                                  # rows behind the end are not touched
    z[1, 2:] = np.nan
    lp, rk, s, n = ref.sequence_score(z, tar, eos=3)
    assert n.tolist() == [3, 2, 5]
    assert np.allclose(lp[0], np.log([.2, .3, .4, 1, 1]), atol=1e-14) and (lp[0, 3:] == 0).all()
    assert rk.tolist() == [[2, 1, 0, -1, -1], [2, 1, -1, -1, -1], [2, 1, 1, 2, 1]]
    assert s == pytest.approx([math.log(.2 * .3 * .4), math.log(.2 * .3), math.log(.2 * .3 * .3 * .2 * .3)], abs=1e-13)
    # n_b = 0: nothing scored, the sum is 0
    lp, rk, s, n = ref.sequence_score(z[:1], np.zeros((1, T), np.int64), eos=3)
    assert n[0] == 0 and s[0] == 0.0 and (rk == -1).all() and (lp == 0).all()
    # the float32 sequential sum: one rounding per position
    vals = np.array([-1.1, -2.7, -0.3], np.float32)
    want = np.float32(np.float32(np.float32(0) + vals[0]) + vals[1])
    assert ref.sequential_sum_f32(vals, 2) == want and ref.sequential_sum_f32(vals, 0) == 0
    assert ref.sequential_sum_f32(np.array([-1.0, -np.inf, -2.0], np.float32), 3) == -np.inf


# ---------------------------------------------------------------- 2. against the oracle's reconstruction loss
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_against_the_oracle_loss(seed):
    """On well-formed rows (tokens, EOS, then only PAD) the masked mean of builders/losses.py:26-41 is -sum_b seq_logp[b] / (B (L - 1))."""
    rng = np.random.RandomState(seed)
    B, T, V, eos = 6, 23, 52, 51
    real = np.zeros((B, T), np.int64)
    for b, n in enumerate([1, 5, 23, 12, 22, 2]):                      # EOS at position n - 1
        real[b, :n - 1] = rng.randint(1, eos - 1, size=n - 1)
        real[b, n - 1] = eos
    pred = rng.randn(B, T, V) * 3.0
    loss, _ = oracle.recon_loss_fwd(real, pred)
    lp, rk, s, n = ref.sequence_score(pred, real, eos)
    assert n.tolist() == [1, 5, 23, 12, 22, 2]
    assert -s.sum() / (B * T) == pytest.approx(loss, rel=1e-12)
    hit = (pred.argmax(-1) == real) & (real != 0)                      # builders/keras_metrics.py:25 on the scored positions
    assert np.array_equal(rk == 0, hit)


# ---------------------------------------------------------------- 3. the host side of Transformer.score
def _fake_engine(calls, V=11, eos=EOS):
    """score_chunk made of the restatement: logits that depend on (input row, position) only, so a row's result cannot depend on
    its chunk; records every call."""
    def score_chunk(inp, tar, m):
        B, L = inp.shape
        assert tar.shape == (B, L) and inp.dtype == np.int64 and tar.dtype == np.int64
        calls.append((inp.copy(), tar.copy(), m))
        z = np.zeros((B, L - 1, V))
        for b in range(B):
            rng = np.random.RandomState(int(inp[b].sum()) % 9973)
            z[b] = rng.randn(L - 1, V)
        lp, rk, s, n = ref.sequence_score(z, tar[:, 1:], eos)
        return lp.astype(np.float32), rk.astype(np.int32), s.astype(np.float32), n.astype(np.int32)     # all B rows: the caller cuts
    return score_chunk


def _rows(n, L, rng, eos=EOS):
    x = np.zeros((n, L), np.int64)
    for i in range(n):
        k = rng.randint(2, L - 1)
        x[i, 0] = 9
        x[i, 1:k] = rng.randint(1, 7, size=k - 1)
        x[i, k] = eos
    return x


def test_score_in_chunks_pads_and_concatenates():
    from sketchformer_amd.models.sketchformer import score_in_chunks
    L, B = 10, 4
    x = _rows(2 * B + 3, L, np.random.RandomState(3))
    calls = []
    res = score_in_chunks(x, None, L, B, EOS, _fake_engine(calls))
    assert [c[2] for c in calls] == [4, 4, 3]
    assert all(c[0].shape == (B, L) for c in calls) and (calls[2][0][3] == 0).all() and (calls[2][1][3] == 0).all()   # zero-padded
    assert np.array_equal(calls[1][0], x[4:8]) and np.array_equal(calls[1][1], x[4:8])                              # tar = inp
    n = len(x)
    assert res['logp'].shape == (n,) and res['length'].shape == (n,) and res['complete'].shape == (n,)
    assert res['token_logp'].shape == (n, L - 1) and res['rank'].shape == (n, L - 1) and res['perplexity'].shape == (n,)
    assert res['complete'].dtype == np.bool_ and res['complete'].all()
    # a row's result does not depend on its chunk
    for i in (0, 5, 10):
        one = score_in_chunks(x[i], None, L, B, EOS, _fake_engine([]))
        for k in res:
            assert np.array_equal(one[k][0], res[k][i]), (k, i)
    assert np.allclose(res['perplexity'], np.exp(-res['logp'].astype(np.float64) / res['length']), rtol=1e-12)


def test_score_in_chunks_window_and_complete():
    from sketchformer_amd.models.sketchformer import score_in_chunks
    L, B = 10, 4
    x = _rows(3, L, np.random.RandomState(4))
    tar = np.zeros((3, L + 1), np.int64)                               # the shape predict / sample / beam_search return
    tar[:, 0] = 9
    tar[0, 1:L + 1] = 5
    tar[0, L] = EOS                                                    # EOS in the last column: outside the window
    tar[1, 1:4] = 5
    tar[1, 4] = EOS
    tar[2, 1:L] = 5
    tar[2, L - 1] = EOS                                                # EOS in the last column of the window
    calls = []
    res = score_in_chunks(x, tar, L, B, EOS, _fake_engine(calls))
    assert calls[0][1].shape == (B, L) and np.array_equal(calls[0][1][:3], tar[:, :L])       # the forward gets the first seq_len columns
    assert res['complete'].tolist() == [False, True, True]
    assert res['length'].tolist() == [L - 1, 4, L - 1]                 # scored on what fits
    assert (res['rank'][0] >= 0).all() and np.isfinite(res['logp']).all()
    # seq_len columns work as well; (n, L, 1) token columns of the file loaders too
    same = score_in_chunks(x[..., None], tar[:, :L], L, B, EOS, _fake_engine([]))
    for k in res:
        assert np.array_equal(same[k], res[k]), k
    # length 0: perplexity divides by 1
    tar0 = np.zeros((1, L), np.int64)
    r0 = score_in_chunks(x[:1], tar0, L, B, EOS, _fake_engine([]))
    assert r0['length'][0] == 0 and r0['logp'][0] == 0 and r0['perplexity'][0] == 1.0 and not r0['complete'][0]
    for bad_inp, bad_tar in ((x[:, :L - 1], None), (x, tar[:2]), (x, np.zeros((3, L + 2), np.int64)), (np.zeros((0, L), np.int64), None)):
        with pytest.raises(ValueError):
            score_in_chunks(bad_inp, bad_tar, L, B, EOS, _fake_engine([]))
