"""The decode-step kernels (skf_decode_init, skf_decode_embed, skf_decode_select_tokens, skf_decode_select_continuous) through the
C ABI.  Whole-model decodes compared with the oracle reach them, but pin none of their rules; here each rule has its own assertion:
first-index tie breaking inside a lane and across lanes, sticky EOS, n_valid < B, done_step written once, the non-sticky stop rule of
the continuous form, and byte-for-byte agreement of the host-step and the device-step (step_dev / dyn) forms.

Out of scope: a row of logits that is entirely -inf or NaN.  The selection kernels would then store 2147483647 (read from the code,
not observed); such rows are for the train step's non-finite guard and are not inputs of these kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import entry_point_checks as epc
from entry_point_checks import SENTINEL, close, dev, filled, ptr, stream

pytestmark = pytest.mark.gpu
ELT_RTOL = 2e-5                      # tests/test_gpu_ops.py: element-wise fp32 results
I64, I32, U8 = torch.int64, torch.int32, torch.uint8
TOK_S, BYTE_S, INT_S = -99, 0xAB, 55  # sentinels of the token, mask-byte and int buffers


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    epc.report()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


class State:
    """The buffers a decode loop owns, every cell a sentinel until a kernel writes it."""

    def __init__(self, B, ld, continuous=False):
        self.tokens = None if continuous else filled(B, ld, dtype=I64, value=TOK_S)
        self.cont = filled(B, ld, 5) if continuous else None
        self.mask = filled(B, ld + 3, dtype=U8, value=BYTE_S)
        self.eos_seen = filled(B + 2, dtype=I32, value=INT_S)
        self.done = filled(2, dtype=I32, value=INT_S)
        self.step_dev = filled(2, dtype=I32, value=INT_S)
        self.B, self.ld = B, ld

    def init(self, lib, sos=0, with_step_dev=True):
        lib.call("skf_decode_init", ptr(self.tokens), self.ld, ptr(self.cont), self.ld, ptr(self.mask), self.ld + 3, ptr(self.eos_seen),
                 ptr(self.done), self.B, sos, ptr(self.step_dev) if with_step_dev else None, stream())

    def everything(self):
        return [t.cpu() for t in (self.tokens, self.cont, self.mask, self.eos_seen, self.done) if t is not None]


# ------------------------------------------------------------------ skf_decode_init
@pytest.mark.parametrize("B", [pytest.param(1, id="B1"), pytest.param(300, id="B300-second-trip-of-256-threads")])
@pytest.mark.parametrize("mode,sos", [pytest.param("tokens", 0, id="tokens-sos-is-pad"), pytest.param("tokens", 7, id="tokens-sos7"),
                                      pytest.param("continuous", 0, id="continuous")])
def test_decode_init(lib, B, mode, sos):
    ld = 6
    for with_step_dev in (True, False):
        s = State(B, ld, continuous=(mode == "continuous"))
        s.init(lib, sos, with_step_dev)
        mask = s.mask.cpu().numpy()
        if mode == "tokens":
            tok = s.tokens.cpu().numpy()
            assert (tok[:, 0] == sos).all() and (tok[:, 1:] == TOK_S).all()
            assert (mask[:, 0] == (1 if sos == 0 else 0)).all()
        else:
            c = s.cont.cpu().numpy()
            assert (c[:, 0] == np.array([0, 0, 1, 0, 0], np.float32)).all() and (c[:, 1:] == np.float32(SENTINEL)).all()
            assert (mask[:, 0] == 0).all()
        assert (mask[:, 1:] == BYTE_S).all()                                   # only column 0 is written
        assert s.eos_seen.tolist() == [0] * B + [INT_S] * 2
        assert s.done.tolist() == [-1, INT_S]
        assert s.step_dev.tolist() == ([0, INT_S] if with_step_dev else [INT_S, INT_S])


# ------------------------------------------------------------------ skf_decode_embed
@pytest.mark.parametrize("step", [pytest.param(0, id="step0"), pytest.param(5, id="step5")])
@pytest.mark.parametrize("B", [pytest.param(1, id="B1"), pytest.param(9, id="B9")])
@pytest.mark.parametrize("d", [pytest.param(36, id="d36-one-workgroup-partial"), pytest.param(128, id="d128-several-workgroups")])
def test_decode_embed(lib, d, B, step):
    rng = np.random.RandomState(d + B + step)
    vocab, ld = 11, 8
    table, pos = _f32(rng.uniform(-1, 1, (vocab, d))), _f32(rng.uniform(-1, 1, (ld, d)))
    W, bias = _f32(rng.uniform(-1, 1, (5, d))), _f32(rng.uniform(-1, 1, d))
    tabd, posd, Wd, bd = dev(table), dev(pos), dev(W), dev(bias)
    step_dev = dev([step, INT_S], I32)
    # token form: ids outside [0, vocab) take the row of id 0 (skf.h: both decode paths clamp; skf_embed_fwd stores zeros instead)
    tok = rng.randint(1, vocab, size=(B, ld)).astype(np.int64)
    odd = np.array([-1, vocab, 2 ** 40, vocab - 1, 0], np.int64)
    for ids in ([odd[:B]] if B >= 5 else [odd[k:k + 1] for k in range(5)]):
        tok[:len(ids), step] = ids
        T = dev(tok, I64)
        out = filled(B * d + 5)
        lib.call("skf_decode_embed", ptr(T), None, ld, B, ptr(tabd), vocab, None, None, d, ptr(posd), ptr(step_dev), ptr(out), stream())
        cl = np.where((tok[:, step] < 0) | (tok[:, step] >= vocab), 0, tok[:, step])
        close(out[:B * d].view(B, d), table[cl] * np.sqrt(d) + pos[step], ELT_RTOL, "skf_decode_embed", "tokens")
        assert float(out[B * d:].min()) == float(out[B * d:].max()) == SENTINEL
    # continuous form
    x = _f32(rng.uniform(-1, 1, (B, ld, 5)))
    X = dev(x)
    out = filled(B * d + 5)
    lib.call("skf_decode_embed", None, ptr(X), ld, B, None, 0, ptr(Wd), ptr(bd), d, ptr(posd), ptr(step_dev), ptr(out), stream())
    close(out[:B * d].view(B, d), (x[:, step] @ W + bias) * np.sqrt(d) + pos[step], ELT_RTOL, "skf_decode_embed", "continuous")
    assert float(out[B * d:].min()) == float(out[B * d:].max()) == SENTINEL
    assert step_dev.tolist() == [step, INT_S]


# ------------------------------------------------------------------ skf_decode_select_tokens
EOS = 1


def _token_plan(B, V, n_valid, rng):
    """Four steps of logits (4, B, ld) and the token every row must pick.  Who emits EOS:
      step 0  only the rows >= n_valid - they never count, however many they are;
      step 1  every valid row but the last - with the rows >= n_valid that makes n_valid or more flags, one valid row missing;
      step 2  the last valid row alone - the others emitted earlier and picked something else now: sticky, done_step = 2;
      step 3  nobody - done_step is not written again."""
    ld = V + 3
    x = rng.randn(4, B, ld).astype(np.float32)
    x[:, :, V:] = 100.0                                                        # columns [V, ld): the largest of the row, never read
    x[:, :, EOS] = -50.0
    want = np.zeros((4, B), np.int64)
    for s in range(4):
        for b in range(B):
            emits = (s == 0 and b >= n_valid) or (s == 1 and b < n_valid - 1) or (s == 2 and b == n_valid - 1)
            kind = (b + s) % 4
            if emits:
                x[s, b, EOS] = 50.0; want[s, b] = EOS
            elif kind == 0 and V > 66:                                          # same lane: j and j + 64
                x[s, b, 2] = x[s, b, 66] = 40.0; want[s, b] = 2
            elif kind <= 1:                                                     # two lanes
                x[s, b, 2] = x[s, b, 4] = 40.0; want[s, b] = 2
            elif kind == 2:                                                     # the maximum at index 0 (and again at 3, at 64): PAD, mask byte
                x[s, b, 0] = x[s, b, 3] = 40.0; want[s, b] = 0
                if V > 64:
                    x[s, b, 64] = 40.0                                          # lane 0 again, on its second trip
            else:
                want[s, b] = int(np.argmax(x[s, b, :V]))
    assert np.array_equal(want, x[:, :, :V].argmax(-1))                          # np.argmax: first index on ties
    return x, want


@pytest.mark.parametrize("V", [pytest.param(5, id="V5-partial-wave"), pytest.param(64, id="V64-one-trip"),
                               pytest.param(65, id="V65-second-trip-lane0"), pytest.param(1004, id="V1004-sixteen-trips")])
@pytest.mark.parametrize("B,n_valid", [pytest.param(1, 1, id="B1"), pytest.param(16, 14, id="B16-one-row-per-wave-valid14"),
                                       pytest.param(16, 2, id="B16-valid2-outnumbered"), pytest.param(17, 15, id="B17-wave0-second-row-valid15"),
                                       pytest.param(17, 2, id="B17-valid2-outnumbered"), pytest.param(40, 38, id="B40-three-rows-per-wave-valid38"),
                                       pytest.param(40, 3, id="B40-valid3-outnumbered")])
def test_decode_select_tokens_three_steps(lib, B, n_valid, V):
    """Three steps that decide done_step and a fourth that must not touch it.  A kernel that counted the rows >= n_valid would stop at
    step 0 where they outnumber the valid rows (valid2, valid3) and at step 1 everywhere (B > 1): both must leave done_step at -1."""
    rng = np.random.RandomState(B * 10000 + V + n_valid)
    x, want = _token_plan(B, V, n_valid, rng)
    ld, tok_ld = V + 3, 6
    X = dev(x)
    dyn = dev([n_valid, EOS], I64)
    host, devf = State(B, tok_ld), State(B, tok_ld)
    host.init(lib, 7); devf.init(lib, 7)
    seen = np.zeros(B, np.int64)
    dones = []
    for s in range(4):
        lib.call("skf_decode_select_tokens", ptr(X[s]), ld, B, V, n_valid, s, EOS, ptr(host.tokens), tok_ld, ptr(host.mask), tok_ld + 3,
                 ptr(host.eos_seen), ptr(host.done), None, None, stream())
        lib.call("skf_decode_select_tokens", ptr(X[s]), ld, B, V, -5, -5, -5, ptr(devf.tokens), tok_ld, ptr(devf.mask), tok_ld + 3,
                 ptr(devf.eos_seen), ptr(devf.done), ptr(devf.step_dev), ptr(dyn), stream())
        seen |= (want[s] == EOS)                                               # sticky
        if B > 1 and s == 0:
            assert seen[n_valid:].all() and not seen[:n_valid].any()            # only the rows >= n_valid have emitted
        if B > 1 and s == 1:
            assert seen.sum() >= n_valid and not seen[n_valid - 1]              # n_valid flags or more, a valid row still missing
        tok, mask = host.tokens.cpu().numpy(), host.mask.cpu().numpy()
        assert np.array_equal(tok[:, 1:s + 2], want[:s + 1].T) and (tok[:, 0] == 7).all() and (tok[:, s + 2:] == TOK_S).all()
        assert np.array_equal(mask[:, 1:s + 2], (want[:s + 1].T == 0).astype(np.uint8)) and (mask[:, s + 2:] == BYTE_S).all()
        assert host.eos_seen.tolist() == list(seen) + [INT_S] * 2
        assert host.done.tolist()[1] == INT_S
        dones.append(host.done.tolist()[0])
        assert devf.step_dev.tolist() == [s + 1, INT_S]                         # the device form advances its own step
        for a, b_ in zip(host.everything(), devf.everything()):
            assert torch.equal(a, b_)                                           # every output byte
    assert dones == [-1, -1, 2, 2], dones


def test_decode_select_tokens_refusals(lib):
    B, V, tok_ld = 4, 8, 6
    X = dev(np.zeros((B, V)))
    s = State(B, tok_ld)
    s.init(lib, 7)
    before = s.everything()

    def go(n_valid, step, step_dev, dyn):
        lib.call("skf_decode_select_tokens", ptr(X), V, B, V, n_valid, step, EOS, ptr(s.tokens), tok_ld, ptr(s.mask), tok_ld + 3,
                 ptr(s.eos_seen), ptr(s.done), step_dev, dyn, stream())
    for bad in ((B, tok_ld - 1, None, None),            # step + 1 >= tok_ld
                (B + 1, 0, None, None),                 # n_valid > B
                (B, 0, ptr(s.step_dev), None)):         # step_dev without dyn
        with pytest.raises(lib.SkfError):
            go(*bad)
    for a, b_ in zip(before, s.everything()):
        assert torch.equal(a, b_)


# ------------------------------------------------------------------ skf_decode_select_continuous
def _pen_plan(B, n_valid, rng):
    """Four steps of predictions (4, B, ld = 7).  Who picks state 2 (end of sketch):
      step 0  only the rows >= n_valid - they never count;
      step 1  they again and every valid row but the last - n_valid picks or more, one valid row missing;
      step 2  every valid row - done_step = 2;
      step 3  every valid row but the last - the rule is not sticky, but done_step is written once."""
    x = rng.uniform(-1, 1, (4, B, 7)).astype(np.float32)
    x[:, :, 5:] = 100.0
    fin = np.zeros((4, B), bool)
    for s in range(4):
        for b in range(B):
            f = [b >= n_valid, b >= n_valid or b < n_valid - 1, b < n_valid, b < n_valid - 1][s]
            fin[s, b] = f
            base = np.float32(rng.uniform(-2, 2))
            if f:
                gap = 30.0 if b % 2 == 0 else 8.0                               # softmax 1.0f exactly (mask byte) / 0.9993 (no mask byte)
                x[s, b, 2:5] = [base - gap, base - gap, base]
            elif (b + s) % 3 == 0:
                x[s, b, 2:5] = base                                             # equal pen logits: state 0
            elif (b + s) % 3 == 1:
                x[s, b, 2:5] = [base - 1, base, base]                           # states 1 and 2 equal: state 1, not the end
            else:
                x[s, b, 2:5] = [base, base - 3, base - 0.5]
    return x, fin


@pytest.mark.parametrize("B,n_valid", [pytest.param(1, 1, id="B1"), pytest.param(257, 255, id="B257-second-trip-of-256-threads-valid255"),
                                       pytest.param(257, 3, id="B257-valid3-outnumbered")])
def test_decode_select_continuous_four_steps(lib, B, n_valid):
    """A kernel that counted the rows >= n_valid would stop at step 0 where they outnumber the valid rows (valid3) and at step 1
    everywhere (B > 1): both must leave done_step at -1."""
    rng = np.random.RandomState(B + n_valid)
    x, fin = _pen_plan(B, n_valid, rng)
    if B > 1:
        assert fin[0, n_valid:].all() and not fin[0, :n_valid].any()
        assert fin[1].sum() >= n_valid and not fin[1, n_valid - 1]
    X = dev(x)
    ld_rows = 7
    dyn = dev([n_valid, 0], I64)
    host, devf = State(B, ld_rows, continuous=True), State(B, ld_rows, continuous=True)
    host.init(lib); devf.init(lib)
    dones = []
    for s in range(4):
        lib.call("skf_decode_select_continuous", ptr(X[s]), 7, B, n_valid, s, ptr(host.cont), ld_rows, ptr(host.mask), ld_rows + 3,
                 ptr(host.done), None, None, stream())
        lib.call("skf_decode_select_continuous", ptr(X[s]), 7, B, -5, -5, ptr(devf.cont), ld_rows, ptr(devf.mask), ld_rows + 3,
                 ptr(devf.done), ptr(devf.step_dev), ptr(dyn), stream())
        z = x[s, :, 2:5].astype(np.float64)
        p = np.exp(z - z.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
        row = host.cont[:, s + 1]
        assert torch.equal(row[:, :2].cpu(), torch.as_tensor(x[s, :, :2]))       # x, y are copied
        close(row[:, 2:], p, ELT_RTOL, "skf_decode_select_continuous", "softmax(pen)")
        got = row[:, 2:].cpu().numpy()
        assert np.array_equal(got.argmax(-1) == 2, fin[s]) and (got[~fin[s]].argmax(-1) < 2).all()
        flat = np.ptp(x[s, :, 2:5], axis=-1) == 0
        assert (got[flat].argmax(-1) == 0).all()                                # equal pen logits pick state 0
        masked = fin[s] & (np.arange(B) % 2 == 0)                               # gap 30: the third probability is 1.0f; gap 8: it is not
        assert np.array_equal(got[:, 2] == np.float32(1.0), masked)
        assert np.array_equal(host.mask[:, s + 1].cpu().numpy(), masked.astype(np.uint8))
        assert (host.mask[:, s + 2:].cpu().numpy() == BYTE_S).all() and (host.cont[:, s + 2:].cpu().numpy() == np.float32(SENTINEL)).all()
        assert host.done.tolist()[1] == INT_S
        dones.append(host.done.tolist()[0])
        assert devf.step_dev.tolist() == [s + 1, INT_S]
        for a, b_ in zip(host.everything(), devf.everything()):
            assert torch.equal(a, b_)
    assert dones == [-1, -1, 2, 2], dones
    assert host.eos_seen.tolist() == [0] * B + [INT_S] * 2         # the continuous form keeps no EOS flags
