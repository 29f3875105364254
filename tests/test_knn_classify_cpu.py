"""CPU: the fp64 oracle of the weighted kNN classifier (tests/knn_classify_oracle.py) against scikit-learn's brute-force search, its tie and NaN rules, the proof -
in fp64 only - that the inputs of tests/test_gpu_knn_classify.py stay under the caps that file excuses (so whatever keeps the GPU tests inside them is the
kernels, not the data), the new entry points' declarations and the command line's new task."""
import os
import re

import numpy as np
import pytest

import knn_classify_oracle as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ssv_knn_search_workspace_bytes", "ssv_knn_search", "ssv_knn_vote")
# (blob shape, k) of the end-to-end GPU test: k = n is left out at (257, 1500, 36, 100), where the fp64 share of near-tied votes passes the 1 % cap
E2E_CASES = tuple((i, k) for i in range(len(kc.BLOB_SHAPES)) for k in kc.KS + ((kc.BLOB_SHAPES[i][1],) if i == 0 else ()))


@pytest.mark.parametrize("index", range(len(kc.BLOB_SHAPES)))
def test_oracle_search_agrees_with_sklearn_brute_force(index):
    neighbors = pytest.importorskip("sklearn.neighbors")
    bank, _, queries, _ = kc.blobs(index)
    b, q = bank.astype(np.float64), queries.astype(np.float64)
    # inner-product search as a Euclidean one: |(q, 0) - (b, sqrt(M^2 - |b|^2))|^2 = |q|^2 + M^2 - 2 q.b
    nb = (b * b).sum(1)
    big = nb.max() * (1 + 1e-9)
    nn = neighbors.NearestNeighbors(n_neighbors=200, algorithm="brute").fit(np.hstack([b, np.sqrt(big - nb)[:, None]]))
    _, got = nn.kneighbors(np.hstack([q, np.zeros((q.shape[0], 1))]))
    sim, idx = kc.search(queries, bank, 200)
    s = kc.similarities(queries, bank)
    assert np.abs(np.take_along_axis(s, got, axis=1) - sim).max() <= 1e-12          # the same similarities, place by place
    clear = np.ones_like(idx, bool)                                                  # places whose neighbours in the order are further than 1e-9 away
    gap = sim[:, :-1] - sim[:, 1:]
    clear[:, :-1] &= gap > 1e-9
    clear[:, 1:] &= gap > 1e-9
    assert clear.mean() > 0.99 and np.array_equal(got[clear], idx[clear])
    assert (np.diff(sim, axis=1) <= 0).all()


def test_oracle_order_rule():
    s = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 0.0, -0.0, np.nan, 2.0]])
    assert kc.order(s).tolist() == [[1, 3, 8, 0, 5, 6, 4, 2, 7]]                    # ties to the lower index, -0 == +0, NaNs last by index, behind -inf
    bank = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0]])
    sim, idx = kc.search(np.array([[0.0, 0.0], [2.0, 0.0]]), bank, 3)
    assert idx.tolist() == [[0, 1, 2], [0, 2, 1]] and sim.tolist() == [[0.0, 0.0, 0.0], [2.0, 2.0, 0.0]]


def test_oracle_vote_rule():
    sim = np.array([[0.9, 0.8, 0.8, 0.1], [0.5, 0.5, np.nan, np.nan]])
    idx = np.array([[0, 1, 2, 3], [3, 2, 1, 7]])
    labels = np.array([2, 1, 1, 0])
    pred, scores = kc.vote(sim, idx, labels, 3, 0.1, topn=3)
    it = kc.inv_temp32(0.1)
    assert np.allclose(scores[0], [np.exp(-0.8 * it), 2 * np.exp(-0.1 * it), 1.0], rtol=1e-15)
    assert pred[0].tolist() == [2, 1, 0]
    assert scores[1].tolist() == [1.0, 1.0, 0.0] and pred[1].tolist() == [0, 1, 2]  # NaN entries and the index 7 outside the bank are not counted; ties to the lower class
    s32 = kc.vote_scores_torch(sim[:1], idx[:1], labels, 3, it, __import__("torch").float64).numpy()
    assert np.allclose(s32, scores[:1], rtol=1e-15)


def test_integer_family_has_straddling_ties_and_no_tied_votes():
    bank, yb, queries, yq = kc.integers()
    s = kc.similarities(queries, bank)
    assert np.array_equal(s, np.round(s)) and np.abs(s).max() < 2 ** 10             # exact in fp32 and in six bf16 piece products
    for k, lo in ((1, 0.05), (20, 0.3), (200, 0.5)):
        share = float(kc.straddling_ties(s, k).mean())
        print(f"integer family k={k}: {share:.1%} of the queries have a tie group across the k-th place")
        assert share >= lo, (k, share)
    for k in kc.KS + (bank.shape[0],):
        res = kc.classify(bank, yb, queries, yq, k, kc.INT_T, kc.INT_SHAPE[3])
        two = -np.partition(-res["scores"], 1, axis=1)[:, :2]
        assert (two[:, 0] > two[:, 1]).all(), k                                      # no query has tied class scores
        assert (kc.relative_margin(res["scores"]) > kc.MU).all(), k


@pytest.mark.parametrize("index,k", E2E_CASES)
def test_blob_votes_are_not_near_ties(index, k):
    """The shares of queries the GPU tests may excuse, computed in fp64 alone: at most 1 %.  Vote test: relative margin below MU.  End-to-end test: below
    2 tau_i / T + MU (a similarity moves by at most tau_i, a weight ratio by exp(2 tau_i / T))."""
    bank, yb, queries, yq = kc.blobs(index)
    c = kc.BLOB_SHAPES[index][3]
    res = kc.classify(bank, yb, queries, yq, k, kc.T_DEFAULT, c)
    margin = kc.relative_margin(res["scores"])
    vote_share = float((margin <= kc.MU).mean())
    e2e_share = float((margin <= 2 * kc.tau(queries, bank) / kc.T_DEFAULT + kc.MU).mean())
    print(f"blobs {kc.BLOB_SHAPES[index]} k={k}: under MU {vote_share:.2%}, under 2 tau / T + MU {e2e_share:.2%}, top1 {res['top1']:.3f}")
    assert vote_share <= kc.MAX_EXCUSED and e2e_share <= kc.MAX_EXCUSED


def test_vote_shapes_are_not_near_ties():
    """The four vote shapes of the GPU test, fed with the oracle's own neighbour lists: at most 1 % of the queries under MU, for both temperatures."""
    import test_gpu_knn_classify as gpu
    for case in gpu.VOTE_CASES:
        for temperature in gpu.VOTE_TEMPERATURES:
            sim, idx, labels, c = gpu.vote_inputs(case)
            _, scores = kc.vote(sim, idx, labels, c, temperature)
            share = float((kc.relative_margin(scores) <= kc.MU).mean())
            print(f"vote case {case} T={temperature}: {share:.2%} under MU")
            assert share <= kc.MAX_EXCUSED, (case, temperature, share)


def test_new_entry_points_are_bound_and_declared():
    from ssv_amd import _lib
    header = open(os.path.join(ROOT, "include", "ssv_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
    lim = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SSV_KNN_MAX_(K|D|CLASSES|TOPN)\s+(\d+)", header)}
    assert (lim["K"], lim["D"], lim["CLASSES"], lim["TOPN"]) == (_lib.KNN_MAX_K, _lib.KNN_MAX_D, _lib.KNN_MAX_CLASSES, _lib.KNN_MAX_TOPN) == (1024, 8192, 4096, 8)
    from ssv_amd import ops
    from ssv_amd.models import base
    from ssv_amd.utils import eval_utils
    assert all(hasattr(ops, f) for f in ("knn_search", "knn_vote")) and hasattr(eval_utils, "knn_classify") and hasattr(base.TwoViewTrainer, "knn_classify_validate")
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "knnclassify.hip")).read()
    assert "knnclassify.hip" in open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "Makefile")).read()
    assert set(re.findall(r"atomicAdd\(&(\w+)", src)) == {"hist", "ngt"}                            # integer LDS atomics only


def test_cli_accepts_knn_eval():
    from ssv_amd import main as cli
    assert "knn_eval" in cli.TASKS and "cluster_eval" in cli.TASKS
    args = cli.parse(["-c", "x.yaml", "-m", "resnet18", "-a", "simclr", "-t", "knn_eval", "-l", "ckpt"])
    assert args["task"] == "knn_eval" and args["load"] == "ckpt"
    with pytest.raises(NotImplementedError):                     # an inference task: it needs --load, like the others
        cli.main(["-c", "x.yaml", "-m", "resnet18", "-a", "simclr", "-t", "knn_eval"])


def test_knn_classify_needs_the_gpu(monkeypatch):
    import torch
    from ssv_amd.utils import eval_utils
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    bank, yb, queries, yq = kc.blobs(0)
    with pytest.raises(RuntimeError, match="no HIP device is visible"):
        eval_utils.knn_classify(bank, yb, queries, yq)
