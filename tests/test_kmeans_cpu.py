"""CPU: the fp64 k-means oracle the GPU tests are held to (tests/kmeans_oracle.py) against scikit-learn's Lloyd, its tie and empty-cluster rules, the
command line's new task, the new entry points' declarations, and the proof - in fp64 only - that the assignment cases of tests/test_gpu_kmeans.py are not
near-tie inputs: whatever keeps the GPU test inside its 1 % cap is then the kernel, not the data."""
import os
import re

import numpy as np
import pytest

import kmeans_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("ssv_kmeans_prep_bytes", "ssv_kmeans_workspace_bytes", "ssv_kmeans_assign", "ssv_kmeans_update", "ssv_cluster_votes")


def test_oracle_agrees_with_sklearn_lloyd():
    cluster = pytest.importorskip("sklearn.cluster")
    n, d, k, niter, seed = 1000, 64, 10, 8, 1234
    x, _ = ko.blobs(7, n, d, k, 0.2)
    x64 = x.astype(np.float64)
    run = ko.lloyd(x, k, niter, seed)
    # sklearn's max_iter counts (assign, update) rounds and its labels_ / inertia_ belong to the centres it returns only after convergence; give it the
    # oracle's `niter` rounds and compare on the oracle's own final assignment of sklearn's centres
    sk = cluster.KMeans(n_clusters=k, init=x64[ko.init_rows(seed, n, k)], n_init=1, algorithm="lloyd", tol=0, max_iter=niter).fit(x64)
    labels, dist = ko.assign(x, sk.cluster_centers_)
    assert np.array_equal(labels, run["labels"])
    assert np.array_equal(sk.labels_, run["labels"])
    assert np.abs(sk.cluster_centers_ - run["centroids"]).max() <= 1e-10
    assert abs(sk.inertia_ - run["objective"]) <= 1e-9 * run["objective"]
    assert abs(dist.sum() - run["objective"]) <= 1e-9 * run["objective"]


def test_oracle_ties_go_to_the_lowest_index():
    x, _ = ko.blobs(3, 200, 16, 6, 1.0)
    c = x[ko.init_rows(5, 200, 6)].copy()
    c[5] = c[2]                                                  # bit-identical rows
    labels, dist = ko.assign(x, c)
    assert not (labels == 5).any() and (labels == 2).any()
    # a point exactly half way between two centroids
    labels, _ = ko.assign(np.array([[0.0, 0.0]]), np.array([[3.0, 0.0], [1.0, 0.0], [-1.0, 0.0]]))
    assert labels.tolist() == [1]


def test_oracle_empty_cluster_keeps_its_centroid():
    x = np.array([[0.0, 0.0], [0.0, 2.0], [10.0, 0.0]])
    c = np.array([[0.0, 1.0], [50.0, 50.0], [9.0, 0.0]])
    labels, _ = ko.assign(x, c)
    assert labels.tolist() == [0, 0, 2]
    new = ko.update(x, labels, c)
    assert np.array_equal(new, np.array([[0.0, 1.0], [50.0, 50.0], [10.0, 0.0]]))
    assert np.array_equal(new[1], c[1])


def test_oracle_redo_rule_and_trace():
    x, _ = ko.blobs(7, 1000, 64, 10, 0.2)
    runs = [ko.lloyd(x, 10, 8, 1234 + r) for r in range(2)]
    best = ko.kmeans(x, 10, niter=8, nredo=2, seed=1234)
    want = 0 if runs[0]["objective"] <= runs[1]["objective"] else 1
    assert best["redo"] == want and best["objective"] == runs[want]["objective"]
    # the two starts end in different optima, far apart: an fp32 run cannot pick the other winner by rounding (tests/test_gpu_kmeans.py relies on it)
    assert abs(runs[0]["objective"] - runs[1]["objective"]) > 1e-3 * min(r["objective"] for r in runs)
    for run in runs:
        tr = run["objectives"] + [run["objective"]]
        assert len(run["objectives"]) == 8 and all(b <= a * (1 + 1e-12) for a, b in zip(tr, tr[1:]))


def test_cli_accepts_cluster_eval():
    from ssv_amd import main as cli
    assert "cluster_eval" in cli.TASKS
    args = cli.parse(["-c", "x.yaml", "-m", "resnet18", "-a", "simclr", "-t", "cluster_eval", "-l", "ckpt"])
    assert args["task"] == "cluster_eval" and args["load"] == "ckpt"
    with pytest.raises(NotImplementedError):                     # an inference task: it needs --load, like the others
        cli.main(["-c", "x.yaml", "-m", "resnet18", "-a", "simclr", "-t", "cluster_eval"])


def test_new_entry_points_are_bound_and_declared():
    from ssv_amd import _lib
    header = open(os.path.join(ROOT, "include", "ssv_hip.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
    lim = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SSV_KMEANS_MAX_(K|D)\s+(\d+)", header)}
    assert (lim["K"], lim["D"]) == (_lib.KMEANS_MAX_K, _lib.KMEANS_MAX_D) and lim["K"] >= 1024 and lim["D"] >= 2048
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    assert all(hasattr(ops, f) for f in ("kmeans_assign", "kmeans_update", "cluster_votes"))
    assert all(hasattr(eval_utils, f) for f in ("kmeans", "compute_cluster_accuracy"))


@pytest.mark.parametrize("index", range(len(ko.ALL_CASES)))
def test_assignment_cases_are_not_near_ties(index):
    """The share of rows the GPU test may excuse (fp64 margin below tau_i), per centroid set, computed in fp64 alone: at most 1 %."""
    x, sets = ko.assign_case(index)
    for c in sets:
        _, margin, tau = ko.margins(x, c)
        share = float((margin < tau).mean())
        assert share <= ko.MAX_EXCUSED, (ko.ALL_CASES[index], share)
