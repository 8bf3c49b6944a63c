"""Host side of the token dictionary: the dictionary files and the Tokenizer's .npz branch, the loader of
prep_data/sketch_token/create_token_dict.py, and the seeded initialisations of sketchformer_amd.kmeans (no GPU)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")))


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("create_token_dict", os.path.join(ROOT, "prep_data", "sketch_token", "create_token_dict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Fitted(object):
    def __init__(self, centers, inertia=1.5, n_iter=7):
        self.cluster_centers_, self.inertia_, self.n_iter_, self.labels_ = centers, inertia, n_iter, None


def _golden_centers():
    c = np.frombuffer(bytes.fromhex(G["dict_tokenizer_centers"]["hex"]), dtype=np.float32).reshape(-1, 2)
    assert hashlib.sha256(c.tobytes()).hexdigest() == G["dict_tokenizer_centers"]["sha256"]
    return c.copy()


def test_npz_dictionary_round_trip(tmp_path):
    from sketchformer_amd import kmeans
    c = _golden_centers()
    path = kmeans.save_dictionary(str(tmp_path / "sub" / "dict.npz"), _Fitted(c, inertia=0.125, n_iter=42))
    with np.load(path) as z:                                       # numpy alone reads it
        assert sorted(z.files) == ["cluster_centers", "inertia", "n_iter"]
        assert z["cluster_centers"].dtype == np.float32 and float(z["inertia"]) == 0.125 and int(z["n_iter"]) == 42
    back = kmeans.load_centers(path)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), c.view(np.uint32))
    with pytest.raises(ValueError):
        kmeans.save_dictionary(str(tmp_path / "bad.npz"), _Fitted(np.zeros((4, 3), np.float32)))


def test_tokenizer_npz_branch_gives_the_golden_tokens(tmp_path):
    """The golden cases were encoded by the reference on a pickled dictionary with these centres: the .npz branch (numpy nearest
    centre, first minimum) gives the same ids, tokens and decoded strokes."""
    from sketchformer_amd import kmeans
    from sketchformer_amd.utils import Tokenizer
    path = kmeans.save_dictionary(str(tmp_path / "dict.npz"), _Fitted(_golden_centers()))
    tok = Tokenizer(path)
    assert tok.dict is None
    assert {k: getattr(tok, k) for k in ("PAD", "SEP", "SOS", "EOS", "VOCAB_SIZE")} == G["dict_tokenizer_ids"]
    cap = Tokenizer(path, max_seq_len=16)
    for case in G["dict_tokenizer"]:
        s = np.array(case["stroke3"], dtype=np.float32)
        assert tok.encode(s.copy()).tolist() == case["tokens"]
        assert tok.encode(s.copy(), seq_len=len(s) + 12).tolist() == case["tokens_seq_len"]
        assert cap.encode(s.copy()).tolist() == case["tokens_max16"]
        assert np.array_equal(np.asarray(tok.decode(case["tokens"]), dtype=np.float64), np.array(case["decoded"]))


def test_pkl_dictionary_is_a_sklearn_kmeans(tmp_path):
    pytest.importorskip("sklearn")
    import pickle
    from sketchformer_amd import kmeans
    c = _golden_centers()
    path = kmeans.save_dictionary(str(tmp_path / "dict.pkl"), _Fitted(c, inertia=2.0, n_iter=9))
    with open(path, "rb") as f:
        km = pickle.load(f)
    assert type(km).__name__ == "KMeans" and km.cluster_centers_.dtype == np.float32 and np.array_equal(km.cluster_centers_, c)
    assert km.inertia_ == 2.0 and km.n_iter_ == 9 and km.n_features_in_ == 2
    assert np.array_equal(km.predict(c[:50]), np.arange(50))
    assert np.array_equal(kmeans.load_centers(path), c)


def test_script_normalise_and_split(script):
    # width 2003 after the clamp -> every offset / 2003; the pen column is clamped with the rest and stays 0 / 1
    s = np.array([[10, 0, 0], [2000, 5, 1], [3, 3, 0], [1, 1, 1], [0, -2000, 0], [1, 1, 1]], dtype=np.int16)
    n = script.normalize_sketch(s)
    assert n.dtype == np.float32 and np.array_equal(n[:, 2], s[:, 2])
    clamped = np.clip(s[:, :2], -1000, 1000).astype(np.float32)
    xs = np.concatenate([[0], np.cumsum(clamped[:, 0])]); ys = np.concatenate([[0], np.cumsum(clamped[:, 1])])
    dim = max(xs.max() - xs.min(), ys.max() - ys.min(), 1)
    assert dim == 1015.0
    want = clamped.copy(); want /= dim
    assert np.array_equal(n[:, :2], want)
    # a sketch smaller than one unit is not blown up: max(w, h, 1) = 1
    tiny = np.array([[0.25, 0.5, 0], [0.25, -0.25, 1]], dtype=np.float32)
    assert np.array_equal(script.normalize_sketch(tiny), tiny)
    # pen lifts at rows 1, 3, 5 -> successors 2, 4 (the successor of the last lift is dropped, here it is past the end)
    hold, lift = script.split_offsets(n)
    assert np.array_equal(lift, n[[2, 4], :2]) and np.array_equal(hold, n[[0, 1, 3, 5], :2])
    # the last lift is not the last row: its successor stays with the pen-hold group, like the reference's [:-1]
    s2 = np.array([[1, 0, 0], [1, 0, 1], [1, 0, 0], [1, 0, 1], [1, 0, 0]], dtype=np.float32)
    hold2, lift2 = script.split_offsets(s2)
    assert len(lift2) == 1 and len(hold2) == 4


def _class_file(path, rng, n_sketches):
    train = np.empty(n_sketches, dtype=object)
    for i in range(n_sketches):
        n = rng.randint(6, 15)
        sk = np.zeros((n, 3), dtype=np.int16)
        sk[:, :2] = rng.randint(-60, 61, size=(n, 2))
        sk[rng.choice(n - 1, 2, replace=False), 2] = 1
        sk[-1, 2] = 1
        train[i] = sk
    other = np.empty(1, dtype=object)
    other[0] = np.full((4, 3), 999, dtype=np.int16)             # must not be read
    np.savez(path, train=train, valid=other, test=other)
    return train


def test_script_loader_and_subsample(script, tmp_path):
    rng = np.random.RandomState(5)
    files, sketches = [], []
    for name in ("cat", "dog"):
        files.append(str(tmp_path / (name + ".npz")))
        sketches += list(_class_file(files[-1], rng, 20))
    p0, p1 = script.load_data(files, verbose=False)
    assert p0.dtype == p1.dtype == np.float32 and p0.shape[1] == p1.shape[1] == 2
    assert len(p0) + len(p1) == sum(len(s) for s in sketches)      # only the train split, every point once
    assert len(p1) == 2 * len(sketches)                              # three lifts per sketch, the last one has no successor
    assert np.abs(np.r_[p0, p1]).max() <= 1.0                       # an offset is no longer than the bounds it was divided by
    want0 = np.concatenate([script.split_offsets(script.normalize_sketch(s))[0] for s in sketches])
    assert np.array_equal(p0, want0)
    # --n-samples is honoured: 100 samples at p1_ratio 0.2 = 80 pen-hold + 20 pen-lift rows, drawn from their own groups
    data = script.subsample(p0, p1, 100, 0.2, seed=1, verbose=False)
    assert data.shape == (100, 2)
    rows = lambda a: set(map(bytes, np.ascontiguousarray(a)))
    assert rows(data[:80]) <= rows(p0) and rows(data[80:]) <= rows(p1)
    assert np.array_equal(data, script.subsample(p0, p1, 100, 0.2, seed=1, verbose=False))
    assert not np.array_equal(data, script.subsample(p0, p1, 100, 0.2, seed=2, verbose=False))
    # a group smaller than its share is kept whole; ratio 0 keeps everything
    big = script.subsample(p0, p1, 2 * len(p0), 0.25, seed=0, verbose=False)      # shares: 1.5 len(p0) and 0.5 len(p0) > len(p1)
    assert len(p1) < len(p0) // 2 and np.array_equal(big, np.r_[p0, p1])
    assert len(script.subsample(p0, p1, 10, 0.0, verbose=False)) == len(p0) + len(p1)


def test_script_unknown_method_exits_1(script, capsys):
    with pytest.raises(SystemExit) as e:
        script.main(["--dataset-dir", "nowhere", "-m", "mini-batch-k-means"])
    assert e.value.code == 1
    assert "Unsupported clustering method: mini-batch-k-means" in capsys.readouterr().out
    d = script.build_parser().parse_args(["-m", "k-means"])          # the reference's flags and defaults
    assert (d.vocab_size, d.n_samples, d.method, d.p1_ratio) == (1000, 5000000, "k-means", 0.2)
    assert (d.class_list, d.target_file) == ("prep_data/quickdraw/list_quickdraw.txt", "prep_data/sketch_token/token_dict.pkl")
    assert (d.n_init, d.max_iter, d.tol, d.seed) == (10, 500, 1e-6, 0)


@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_host_inits_are_distinct_seeded_and_reproducible(init):
    from sketchformer_amd import kmeans
    pts = np.random.RandomState(0).normal(0, 0.08, size=(3000, 2)).astype(np.float32)
    K = 40                                                           # 64 K < N: k-means++ works on a subsample
    a = kmeans.init_centers(pts, K, init, seed=3)
    assert a.shape == (K, 2) and a.dtype == np.float32
    assert len(np.unique(a, axis=0)) == K                            # K distinct rows ...
    assert set(map(bytes, a)) <= set(map(bytes, pts))                # ... of the data
    assert np.array_equal(a, kmeans.init_centers(pts, K, init, seed=3))
    assert not np.array_equal(a, kmeans.init_centers(pts, K, init, seed=4))
    with pytest.raises(ValueError):
        kmeans.init_centers(pts[:10], 11, init, seed=0)


def test_kmeanspp_never_draws_a_duplicate_row():
    """Data with fewer distinct values than centres: the D^2 weights run out, the rest comes from rows not chosen yet."""
    from sketchformer_amd import kmeans
    pts = np.repeat(np.array([[0, 0], [1, 0], [0, 1]], dtype=np.float32), 4, axis=0)
    idx = kmeans.kmeanspp_indices(pts, 7, np.random.RandomState(0))
    assert len(set(idx.tolist())) == 7
    assert len(np.unique(pts[idx[:3]], axis=0)) == 3                 # the three distinct values first
    with pytest.raises(ValueError):
        kmeans.init_centers(pts, 3, "k-medoids", seed=0)
