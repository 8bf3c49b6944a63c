"""Latent interpolation on the device: skf_interpolate_f32 against an fp64 restatement of the reference's slerp, its exact
cases, the lerp mode, the refusals, Transformer.interpolate and the interpolations-for-mturk experiment end to end."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _steps(T):
    return torch.linspace(0, 1, T, dtype=torch.float32)


def _ref_slerp(a, b, t32):
    """utils/skt_tools.py:18-25 of the reference in float64, per pair and step, at float64(t32): normalise, arccos of the dot
    product, the sin weights, `return p0` when sin(omega) < 1e-6.  -> (out (P, T, d), w0 (P, T), w1 (P, T), sin omega (P,))."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    P, d = a.shape
    T = len(t32)
    out, w0, w1, so = np.empty((P, T, d)), np.empty((P, T)), np.empty((P, T)), np.empty(P)
    for p in range(P):
        omega = np.arccos(np.dot(a[p] / np.linalg.norm(a[p]), b[p] / np.linalg.norm(b[p])))
        so[p] = np.sin(omega)
        for j in range(T):
            t = np.float64(t32[j])
            if so[p] < 1e-6:
                w0[p, j], w1[p, j] = 1.0, 0.0
                out[p, j] = a[p]
            else:
                w0[p, j], w1[p, j] = np.sin((1.0 - t) * omega) / so[p], np.sin(t * omega) / so[p]
                out[p, j] = w0[p, j] * a[p] + w1[p, j] * b[p]
    return out, w0, w1, so


def _pair(seed, P, d):
    r = np.random.RandomState(seed)
    return r.randn(P, d).astype(np.float32), (3.0 * r.randn(P, d)).astype(np.float32)


def _run(a, b, t, mode='slerp'):
    from sketchformer_amd import ops
    return ops.interpolate(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), t, mode).cpu().numpy()


# ------------------------------------------------------------------ 1. slerp numerics
@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("P", [1, 5, 9])
@pytest.mark.parametrize("d", [4, 36, 256, 260])
def test_slerp_against_fp64_restatement(d, P, T):
    """Bound per element: 4 * 2^-24 * (|w0| |a_i| + |w1| |b_i|) - three fp32 roundings (each weight, the product, the fused
    add), each at most 2^-24 of its term, and one more for the fp64 scalar path.  Meant for sin(omega) >= 1e-3 (near the
    antiparallel pole the weights grow like 1 / sin(omega)); every pair here has to meet that, none is skipped."""
    seed = ([4, 36, 256, 260].index(d) * 6 + [1, 5, 9].index(P) * 2 + [1, 10].index(T)) % 20
    a, b = _pair(seed, P, d)
    t = _steps(T)
    got = _run(a, b, t)
    ref, w0, w1, so = _ref_slerp(a, b, t.numpy())
    assert got.shape == (P, T, d) and got.dtype == np.float32
    assert (so >= 1e-3).all(), so.min()
    bound = 4 * EPS * (np.abs(w0)[:, :, None] * np.abs(a.astype(np.float64))[:, None, :]
                       + np.abs(w1)[:, :, None] * np.abs(b.astype(np.float64))[:, None, :])
    err = np.abs(got.astype(np.float64) - ref)
    print("d %d P %d T %d: worst error / bound %.3f, smallest sin(omega) %.3f" % (d, P, T, (err / np.maximum(bound, 1e-300)).max(), so.min()))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()


# ------------------------------------------------------------------ 2. exact cases
def test_endpoints_are_the_inputs():
    a, b = _pair(3, 9, 260)
    for T in (2, 10):
        got = _run(a, b, _steps(T))
        assert np.array_equal(got[:, 0], a) and np.array_equal(got[:, T - 1], b)


@pytest.mark.parametrize("scale", [1.0, 2.0, -1.0])
def test_parallel_and_antiparallel_pairs_return_a(scale):
    a, _ = _pair(4, 9, 260)
    got = _run(a, (scale * a).astype(np.float32), _steps(10))
    assert np.array_equal(got, np.broadcast_to(a[:, None, :], got.shape))


def test_lerp_midpoint_of_equal_rows_and_repeatability():
    a, b = _pair(5, 9, 36)
    got = _run(a, a, [0.5], 'lerp')
    assert np.array_equal(got[:, 0], a)
    for mode in ('slerp', 'lerp'):
        one, two = _run(a, b, _steps(10), mode), _run(a, b, _steps(10), mode)
        assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


def test_row_pitch():
    from sketchformer_amd import ops
    P, d, T = 5, 36, 10
    a, b = _pair(6, P, d)
    wa, wb = torch.full((P, d + 12), 7.0, device='cuda'), torch.full((P, d + 4), 7.0, device='cuda')
    wa[:, :d], wb[:, :d] = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    wide = torch.full((P, T, d + 8), -5.0, device='cuda')
    for mode in ('slerp', 'lerp'):
        want = _run(a, b, _steps(T), mode)
        assert np.array_equal(ops.interpolate(wa[:, :d], wb[:, :d], _steps(T), mode).cpu().numpy(), want)
        wide.fill_(-5.0)
        res = ops.interpolate(wa[:, :d], wb[:, :d], _steps(T), mode, out=wide[:, :, :d])
        assert res.data_ptr() == wide.data_ptr()
        assert np.array_equal(wide[:, :, :d].cpu().numpy(), want)
        assert (wide[:, :, d:] == -5.0).all().item()


# ------------------------------------------------------------------ 3. lerp
@pytest.mark.parametrize("d,P", [(4, 1), (36, 9), (260, 5)])
def test_lerp_bits(d, P):
    """The two fp32 operations fmaf(t, b, (1 - t) * a), restated in float64 and rounded once."""
    a, b = _pair(7, P, d)
    t = np.concatenate([_steps(10).numpy(), np.float32([0.3, 0.71, 1.5, -0.25])])
    got = _run(a, b, torch.from_numpy(t), 'lerp')
    one_minus_t = (np.float32(1) - t)[None, :, None]
    first = (one_minus_t * a[:, None, :]).astype(np.float32)                       # fp32 product, rounded
    want = (t.astype(np.float64)[None, :, None] * b.astype(np.float64)[:, None, :] + first.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ 4. refusals
def test_refusals():
    from sketchformer_amd import ops, _lib
    a, b = torch.ones(8, 16, device='cuda'), torch.ones(8, 16, device='cuda')
    with pytest.raises(_lib.SkfError, match="multiple of 4"):
        ops.interpolate(torch.ones(8, 6, device='cuda'), torch.ones(8, 6, device='cuda'), [0.0, 1.0])
    with pytest.raises(_lib.SkfError, match="16-byte aligned"):
        ops.interpolate(torch.ones(8, 18, device='cuda')[:, :16], b, [0.0, 1.0])
    with pytest.raises(_lib.SkfError, match="16-byte aligned"):
        ops.interpolate(torch.ones(8, 20, device='cuda')[:, 1:17], b, [0.0, 1.0])
    with pytest.raises(_lib.SkfError):
        ops.interpolate(a, b, torch.zeros(0, device='cuda'))
    with pytest.raises(_lib.SkfError, match=r"T must be in \[1, 256\]"):
        ops.interpolate(a, b, _steps(257))
    with pytest.raises(ValueError):
        ops.interpolate(a, b, [0.0, 1.0], mode=2)
    with pytest.raises(ValueError):
        ops.interpolate(a, torch.ones(7, 16, device='cuda'), [0.0, 1.0])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. model.interpolate
SMALL = "num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=32,dropout_rate=0.1"


def _model(tmp_path, loader_hps, specific=SMALL, loader="stroke3-synthetic", data_dir=None):
    from sketchformer_amd import models, dataloaders
    Model = models.get_model_by_name("sketch-transformer-tf2")
    Loader = dataloaders.get_dataloader_by_name(loader)
    dataset = Loader(Loader.parse_hparams(loader_hps), data_dir)
    return Model(Model.parse_hparams(base="batch_size=8,num_epochs=1,log_every=4", specific=specific), dataset, str(tmp_path), "it")


@pytest.mark.parametrize("continuous", [False, True])
def test_model_interpolate(tmp_path, continuous):
    from sketchformer_amd import ops
    if continuous:       # attn_version 2: the embedding has lowerdim columns; a non-blind decoder
        model = _model(tmp_path, "max_seq_len=24,n_classes=7,n_samples=64,use_continuous_data=true",
                       SMALL + ",attn_version=2,blind_decoder_mask=false")
    else:
        model = _model(tmp_path, "max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64")
    P, T, B, L = 5, 4, 8, 24
    x_a, _ = model.dataset.get_n_samples_from("valid", P)
    x_b, _ = model.dataset.get_n_samples_from("test", P)
    res = model.interpolate(x_a, x_b, n_steps=T)
    z = res['embedding']
    E = 32 if continuous else 64
    assert z.shape == (P, T, E) and z.dtype == np.float32
    za, zb = model.predict_class(x_a)['embedding'], model.predict_class(x_b)['embedding']
    assert np.array_equal(z[:, 0], za) and np.array_equal(z[:, -1], zb)
    direct = ops.interpolate(torch.from_numpy(za).cuda(), torch.from_numpy(zb).cuda(), _steps(T)).cpu().numpy()
    assert np.array_equal(z.view(np.uint32), direct.view(np.uint32))
    # the same bits through the same chunks: 20 rows = 8 + 8 + 4
    assert res['recon'].shape == ((P, T, L + 1, 5) if continuous else (P, T, L + 1))
    assert res['class'].shape == (P, T) and res['class'].dtype == np.int32
    flat_z = z.reshape(P * T, E)
    flat_r = res['recon'].reshape((P * T,) + res['recon'].shape[2:])
    flat_c = res['class'].reshape(P * T)
    for c in range(3):
        one = model.predict_from_embedding(flat_z[c * B:(c + 1) * B])
        r = np.asarray(one['recon'])
        want = np.zeros((r.shape[0], L + 1) + r.shape[2:], dtype=r.dtype)
        want[:, :r.shape[1]] = r
        assert want.shape[0] == (8, 8, 4)[c]
        assert np.array_equal(flat_r[c * B:(c + 1) * B], want)
        assert np.array_equal(flat_c[c * B:(c + 1) * B], one['class'])
    only_z = model.interpolate(x_a, x_b, n_steps=T, decode=False)
    assert only_z['recon'] is None and only_z['class'] is None and np.array_equal(only_z['embedding'], z)


def test_model_interpolate_needs_a_bottleneck(tmp_path):
    model = _model(tmp_path, "max_seq_len=24,vocab_size=52,n_classes=7,n_samples=64",
                   "num_layers=2,d_model=64,dff=128,num_heads=4,lowerdim=0,do_classification=false")
    x, _ = model.dataset.get_n_samples_from("valid", 3)
    with pytest.raises(ValueError, match="lowerdim"):
        model.interpolate(x, x, n_steps=4)


# ------------------------------------------------------------------ 6. the experiment end to end
def _sketches(rng, n, normalised):
    out = np.empty(n, dtype=object)
    for i in range(n):
        m = rng.randint(5, 16)
        s = np.zeros((m, 3), np.float32)
        s[:, :2] = rng.randint(-20, 20, (m, 2))
        if normalised:
            s[:, :2] /= np.float32(20 * m)                              # the absolute path stays inside [-1, 1]^2
        s[:, 2] = rng.rand(m) < 0.2
        s[-1, 2] = 1
        out[i] = s
    return out


def test_interpolations_for_mturk_experiment(tmp_path):
    from sketchformer_amd import experiments
    rng = np.random.RandomState(0)
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    for name, n in (("train", 16), ("valid", 8), ("test", 8)):
        np.savez(str(data_dir / (name + ".npz")), x=_sketches(rng, n, False), y=rng.randint(0, 3, n))
    np.savez(str(data_dir / "meta.npz"), n_classes=3, n_samples_train=16, class_names=np.array(["a", "b", "c"]), std=1.0)
    model = _model(tmp_path, "token_type=grid,max_seq_len=24", loader="stroke3-distributed", data_dir=str(data_dir))
    sets = {}
    for k, name in enumerate(("source", "intra", "inter")):
        sets[name] = dict(data=_sketches(rng, 3, True), cat=np.array([0, 1, 2]) if name != "inter" else np.array([1, 2, 0]),
                          ids=np.arange(3) + 100 * (k + 1))
        np.savez(str(tmp_path / (name + ".npz")), **sets[name])
    Exp = experiments.get_experiment_by_name("interpolations-for-mturk")
    hps = "source_emb=%s,intra_emb=%s,inter_emb=%s,n_inter=4" % tuple(tmp_path / (n + ".npz") for n in ("source", "intra", "inter"))
    out_dir = Exp(Exp.parse_hparams(hps), "e0", str(tmp_path)).compute(model)
    assert os.path.basename(out_dir) == "interpolations"

    src = np.load(os.path.join(os.path.dirname(out_dir), "reconstructions", "reconstructed_source.npz"), allow_pickle=True)
    assert set(src.files) == {"recon", "cat", "ids"} and len(src["recon"]) == 3
    assert all(np.asarray(s).ndim == 2 and np.asarray(s).shape[1] == 3 for s in src["recon"])
    assert np.array_equal(src["cat"], sets["source"]["cat"]) and np.array_equal(src["ids"], sets["source"]["ids"])

    pre = lambda d: np.squeeze(model.dataset.preprocess_extra_sets_from_interp_experiment(d), axis=-1)   # noqa: E731
    for set_type in ("intra", "inter"):
        names = ["%03d_slerp_%d_%d_%d_%d.svg" % (i, sets["source"]["cat"][i], sets[set_type]["cat"][i], sets["source"]["ids"][i],
                                                   sets[set_type]["ids"][i]) for i in range(3)]
        assert sorted(os.listdir(os.path.join(out_dir, set_type))) == names
        for n in names:
            root = ET.parse(os.path.join(out_dir, set_type, n)).getroot()
            assert len([e for e in root.iter() if e.tag.endswith("path")]) == 4
        saved = np.load(os.path.join(out_dir, set_type + ".npz"), allow_pickle=True)
        assert list(saved["files"]) == names
        assert np.array_equal(saved["cat_dst"], sets[set_type]["cat"]) and np.array_equal(saved["ids_dst"], sets[set_type]["ids"])
        assert np.array_equal(saved["cat_src"], sets["source"]["cat"]) and np.array_equal(saved["ids_src"], sets["source"]["ids"])
        if set_type == "intra":
            direct = model.interpolate(pre(sets["source"]["data"]), pre(sets["intra"]["data"]), 4, 'slerp')
            assert saved["embedding"].shape == (3, 4, 64) and saved["recon"].shape == (3, 4, 25)
            assert np.array_equal(saved["embedding"].view(np.uint32), direct["embedding"].view(np.uint32))
            assert np.array_equal(saved["recon"], direct["recon"])
