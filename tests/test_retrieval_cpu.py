"""Host side of embedding retrieval: the scores against hand-worked cases and a direct loop, the experiment's registration,
and the host-only behaviour of the k-NN entry points (no GPU needed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_average_precision_hand_worked():
    from sketchformer_amd.retrieval import average_precision_at_k
    assert average_precision_at_k(np.array([[True, False, False]]), [1])[0] == 1.0
    assert average_precision_at_k(np.array([[False, True, False, True]]), [2])[0] == pytest.approx((1 / 2 + 2 / 4) / 2)
    assert average_precision_at_k(np.array([[True, True]]), [5])[0] == 1.0              # R > k: the denominator is k
    assert average_precision_at_k(np.array([[False, False, True]]), [1])[0] == pytest.approx(1 / 3)
    assert np.isnan(average_precision_at_k(np.array([[False, False]]), [0])[0])


def test_retrieval_scores_hand_worked():
    from sketchformer_amd.retrieval import retrieval_scores
    gallery_y = np.array([0, 0, 1, 1, 2])
    # query 0 (label 0): ranks rows 0, 2 -> AP (1/1) / min(2, 2) = 0.5; query 1 (label 2): one relevant row, at rank 2 -> 0.5;
    # query 2 (label 9): nothing relevant in the gallery -> not scored
    s = retrieval_scores(np.array([[0, 2], [3, 4], [0, 1]]), np.array([0, 2, 9]), gallery_y)
    assert s['n_queries_scored'] == 2
    assert s['map_at_k'] == pytest.approx(0.5) and s['precision_at_k'] == pytest.approx(0.5) and s['recall_at_1'] == pytest.approx(0.5)
    assert s['per_class_ap'] == {0: pytest.approx(0.5), 2: pytest.approx(0.5)}
    # leave-one-out over the gallery itself: R drops by one, so label 2 (a single row) is no longer scored
    idx = np.array([[1, 2], [0, 2], [3, 0], [2, 0], [0, 1]])
    s = retrieval_scores(idx, gallery_y, gallery_y, exclude_self=True)
    assert s['n_queries_scored'] == 4 and 2 not in s['per_class_ap']
    assert s['map_at_k'] == pytest.approx(1.0) and s['recall_at_1'] == pytest.approx(1.0)
    assert retrieval_scores(idx, gallery_y, gallery_y, exclude_self=False)['n_queries_scored'] == 5
    assert retrieval_scores(idx, gallery_y, gallery_y, exclude_self=False)['map_at_k'] == pytest.approx((4 * 0.5 + 0.0) / 5)


def test_scores_of_exact_ranking_equal_direct_loop():
    from sketchformer_amd.retrieval import retrieval_scores
    r = np.random.RandomState(3)
    Q, G, d, k, C = 40, 300, 16, 12, 6
    centres = r.randn(C, d)
    gy, qy = r.randint(0, C, G), r.randint(0, C + 1, Q)                # label C never occurs in the gallery
    g = (centres[gy] + 0.8 * r.randn(G, d)).astype(np.float32).astype(np.float64)
    q = (np.vstack([centres, np.zeros((1, d))])[qy] + 0.8 * r.randn(Q, d)).astype(np.float32).astype(np.float64)
    D = (q * q).sum(1)[:, None] + (g * g).sum(1)[None, :] - 2.0 * q @ g.T
    idx = np.argsort(D, axis=1, kind='stable')[:, :k]
    aps, precs, r1, per = [], [], [], {}
    for i in range(Q):
        R = int((gy == qy[i]).sum())
        if R == 0:
            continue
        hits, total = 0, 0.0
        for j in range(k):
            if gy[idx[i, j]] == qy[i]:
                hits += 1
                total += hits / (j + 1.0)
        aps.append(total / min(k, R)); precs.append(hits / k); r1.append(float(gy[idx[i, 0]] == qy[i]))
        per.setdefault(int(qy[i]), []).append(aps[-1])
    s = retrieval_scores(idx, qy, gy)
    assert s['n_queries_scored'] == len(aps) < Q
    assert s['map_at_k'] == pytest.approx(np.mean(aps), abs=1e-12)
    assert s['precision_at_k'] == pytest.approx(np.mean(precs), abs=1e-12)
    assert s['recall_at_1'] == pytest.approx(np.mean(r1), abs=1e-12)
    assert set(s['per_class_ap']) == set(per)
    for c, v in per.items():
        assert s['per_class_ap'][c] == pytest.approx(np.mean(v), abs=1e-12)


def test_experiment_is_registered_with_its_defaults():
    from sketchformer_amd import experiments
    Exp = experiments.get_experiment_by_name('sketch-retrieval')
    assert Exp.requires_model is True
    want = dict(batch_size=256, gallery_set='test', query_set='valid', top_k=100, metric='l2', n_queries=0, target_file='retrieval.npz')
    assert dict(Exp.specific_default_hparams().values()) == want
    out = subprocess.run([sys.executable, os.path.join(ROOT, "run-experiment.py"), "sketch-retrieval", "--help-hps"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    for key, val in want.items():
        assert "'%s': %r" % (key, val) in out.stdout, out.stdout


def test_knn_host_only_behaviour():
    import torch
    from sketchformer_amd import build, _lib, ops
    build.build_library(verbose=False)
    lib = _lib.load()
    small, large = lib.skf_knn_workspace_bytes(100, 5000, 10), lib.skf_knn_workspace_bytes(4000, 5000, 10)
    assert 0 < small < large
    assert lib.skf_knn_workspace_bytes(1, 862500, 128) > 0
    assert lib.skf_knn_workspace_bytes(100, 5000, 0) == 0 and lib.skf_knn_workspace_bytes(100, 5000, 129) == 0
    assert lib.skf_knn_workspace_bytes(100, 0, 1) == 0 and lib.skf_knn_workspace_bytes(0, 5000, 1) == 0
    assert lib.skf_knn_workspace_bytes(100, 5, 6) == 0
    # argument checks come before any launch: they answer without a device
    assert lib.skf_knn_topk_f32(None, 8, 4, None, 8, 16, 8, 2, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.skf_last_error()
    assert lib.skf_row_normalize_f32(None, 8, 4, 8, None, 8, None) == -1
    with pytest.raises(_lib.SkfError):
        ops.knn_topk(torch.zeros(4, 8), torch.zeros(16, 8), 2)
    with pytest.raises(_lib.SkfError):
        ops.row_normalize(torch.zeros(4, 8))
    with pytest.raises(ValueError):
        ops.knn_topk(torch.zeros(4, 8), torch.zeros(16, 8), 2, metric='manhattan')
