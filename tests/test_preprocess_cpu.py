"""Device preprocessing, the parts that need no GPU: ragged packing, the device-path predicate against the parent loader's own
fallback, the loader registry, the workspace query, the empty-sketch error - and the two fixtures that give
tests/test_gpu_preprocess.py its teeth, asserted here on the CPU so that the GPU tests cannot pass by accident."""
import itertools

import numpy as np
import pytest

import preprocess_reference as ref
from sketchformer_amd import dataloaders, preprocess
from sketchformer_amd.utils.tokenizer import GridTokenizer, Tokenizer


def _sketches(rng, n, dtype=np.int16):
    out = np.empty(n, dtype=object)
    for i in range(n):
        m = int(rng.randint(1, 40))
        s = np.zeros((m, 3), dtype=dtype)
        s[:, :2] = rng.randint(-30, 31, size=(m, 2))
        s[rng.randint(0, m), 2] = 1
        out[i] = s
    return out


def test_pack_ragged_round_trips():
    rng = np.random.RandomState(0)
    data = _sketches(rng, 37)
    flat, offsets = preprocess.pack_ragged(data)
    assert flat.dtype == np.float32 and flat.shape == (sum(len(s) for s in data), 3) and flat.flags["C_CONTIGUOUS"]
    assert offsets.dtype == np.int64 and offsets.shape == (38,) and offsets[0] == 0 and offsets[-1] == len(flat)
    assert np.all(np.diff(offsets) == [len(s) for s in data])
    for i, s in enumerate(data):
        assert np.array_equal(flat[offsets[i]:offsets[i + 1]], s.astype(np.float32))
    # a list, float64 rows, a fourth column and an empty sketch in the middle
    odd = [np.array([[1.5, -2.0, 0, 9], [0.25, 3.0, 1, 9]]), np.zeros((0, 3)), np.array([[7.0, 8.0, 1.0]])]
    flat, offsets = preprocess.pack_ragged(odd)
    assert offsets.tolist() == [0, 2, 2, 3]
    assert np.array_equal(flat, np.array([[1.5, -2, 0], [0.25, 3, 1], [7, 8, 1]], np.float32))
    flat, offsets = preprocess.pack_ragged([])
    assert flat.shape == (0, 3) and offsets.tolist() == [0]


@pytest.fixture(scope="module")
def dictionary(tmp_path_factory):
    rng = np.random.RandomState(3)
    path = ref.npz_dictionary(tmp_path_factory.mktemp("dict") / "dict.npz", rng.uniform(-0.3, 0.3, size=(12, 2)))
    return Tokenizer(path, max_seq_len=0)


def test_device_path_supported_agrees_with_the_parents_fallback(dictionary, monkeypatch):
    """Over the cross product of the four hparams: the predicate is true exactly where the parent's `preprocess` takes its block
    path (observed on the parent itself, with both of its paths replaced by markers)."""
    parent = dataloaders.get_dataloader_by_name("stroke3-distributed")
    monkeypatch.setattr(parent, "_preprocess_block", lambda self, data, augment: np.zeros((len(data), 1)))
    monkeypatch.setattr(parent, "preprocess_per_sketch", lambda self, data, augment=False: "per-sketch")
    data = _sketches(np.random.RandomState(1), 5)
    seen = set()
    for shuffle, absolute, continuous, token_type in itertools.product((False, True), (False, True), (False, True),
                                                                        ("dictionary", "grid")):
        tok = None if continuous else (dictionary if token_type == "dictionary" else GridTokenizer(resolution=100))
        obj = ref.host_loader(tokenizer=tok, shuffle_stroke=shuffle, use_absolute_strokes=absolute,
                              use_continuous_data=continuous, token_type=token_type)
        block = not isinstance(obj.preprocess(data), str)
        assert preprocess.device_path_supported(obj.hps, tok) == block, (shuffle, absolute, continuous, token_type)
        seen.add(block)
    assert seen == {False, True}
    # a tokenizer that is neither of the two has no block path and no device path
    hps = ref.host_loader(tokenizer=object()).hps
    assert not preprocess.device_path_supported(hps, object())
    assert isinstance(ref.host_loader(tokenizer=object()).preprocess(data), str)


def test_device_loader_is_registered_with_the_parents_hparams():
    dev = dataloaders.get_dataloader_by_name("stroke3-distributed-device")
    parent = dataloaders.get_dataloader_by_name("stroke3-distributed")
    assert dev.name == "stroke3-distributed-device" and issubclass(dev, parent) and dev is not parent
    assert dev.default_hparams().values() == parent.default_hparams().values()
    overridden = {n for n in vars(dev) if not n.startswith("_")} - {"name"}
    assert overridden == {"preprocess"}


def test_workspace_query():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    lib = _lib.load()
    q = lib.skf_sketch_encode_workspace_bytes
    for P, N in ((0, 1), (-1, 1), (1 << 31, 1), (10, 0), (10, -3)):
        assert q(P, N) == 0, (P, N)
    sizes = [q(P, 7) for P in (1, 2, 63, 64, 65, 1000, 100000, (1 << 31) - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 20 * ((1 << 31) - 1)


def test_encode_chunk_refuses_an_empty_sketch_before_the_device(dictionary, monkeypatch):
    import torch
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch.cuda, "Stream", boom)
    data = [np.array([[1, 2, 0], [3, 4, 1]], np.int16), np.zeros((0, 3), np.int16)]
    for tok, over in ((dictionary, {}), (GridTokenizer(resolution=100), {"token_type": "grid"}), (None, {"use_continuous_data": True})):
        hps = ref.host_loader(tokenizer=tok, **over).hps
        with pytest.raises(IndexError):
            preprocess.encode_chunk(data, hps, tok)
    with pytest.raises(ValueError):
        preprocess.encode_chunk(data[:1], ref.host_loader(tokenizer=dictionary, use_absolute_strokes=True).hps, dictionary)


def test_fixture_grid_ids_depend_on_the_summation_order():
    """(a) At least 5 integer sketches whose grid ids under a 64-wide block scan differ from the sequential ones - and the host
    tokenizer is on the sequential side."""
    found, searched = ref.summation_order_sketches()
    assert len(found) >= 5, "only %d of %d sketches depend on the summation order" % (len(found), searched)
    tok = GridTokenizer(resolution=100)
    for s in found:
        nrm = ref.normalise(s)
        seq = ref.grid_ids(nrm, 100, lambda v: np.cumsum(v, dtype=np.float32))
        blk = ref.grid_ids(nrm, 100, ref.block_scan_cumsum_f32)
        assert not np.array_equal(seq, blk)
        enc = tok.encode(nrm)
        host_ids = enc[(enc > 0) & (enc < tok.SEP)]
        assert np.array_equal(host_ids, seq[:len(host_ids)]) and len(host_ids) == len(seq)      # (the last point lifts the pen)


def test_fixture_fp32_distances_tie_where_float64_ones_do_not(dictionary):
    """(b) The fmaf rule of skf_kmeans_assign_f32 returns index 0, the tokenizer's float64 rule index 1."""
    point, centers = ref.tie_fixture()
    assert ref.fmaf_nearest(point, centers).tolist() == [0]
    assert ref.numpy_nearest(point, centers).tolist() == [1]
    tok = Tokenizer.__new__(Tokenizer)
    tok.dict, tok.centers = None, centers.astype(np.float64)
    assert tok.nearest_center(point[:, 0], point[:, 1]).tolist() == [1]
    # the other fixture of the GPU test: a float64 centre that fp32 cannot hold; cast to fp32 the two centres tie and 0 wins
    c64 = np.array([[0.25, 0.0], [-0.25 - 2.0 ** -40, 0.0]]), np.zeros((1, 2), np.float32)
    assert ref.numpy_nearest(c64[1], c64[0]).tolist() == [0]
    c64 = np.array([[-0.25 - 2.0 ** -40, 0.0], [0.25, 0.0]])
    assert ref.numpy_nearest(np.zeros((1, 2), np.float32), c64).tolist() == [1]
    assert ref.numpy_nearest(np.zeros((1, 2), np.float32), c64.astype(np.float32)).tolist() == [0]
