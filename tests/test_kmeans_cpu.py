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


CASE_TABLE = [("assign", i) for i in range(len(ko.ALL_CASES))] + [("form", i) for i in range(len(ko.FORM_CASES))]


@pytest.mark.parametrize("table,index", CASE_TABLE, ids=[str(i) if t == "assign" else f"form{i}" for t, i in CASE_TABLE])
def test_assignment_cases_are_not_near_ties(table, index):
    """The share of rows the GPU test may excuse (fp64 margin below tau_i), per centroid set, computed in fp64 alone: at most 1 %.  For the launch forms of
    tests/test_gpu_kmeans_forms.py also: every centroid of every set wins at least one row in fp64, so a tile, a pass or a register position whose scores were
    never read back would lose rows the reference gives it."""
    x, sets = ko.assign_case(index) if table == "assign" else ko.form_case(index)
    case = (ko.ALL_CASES if table == "assign" else ko.FORM_CASES)[index]
    assert x.shape == case[:2] and all(c.shape == (case[2], case[1]) and c.dtype == np.float32 for c in sets) and len(sets) == 3
    for c in sets:
        _, margin, tau = ko.margins(x, c)
        share = float((margin < tau).mean())
        assert share <= ko.MAX_EXCUSED, (case, share)
        if table == "form":
            wins = np.bincount(ko.assign(x, c)[0], minlength=case[2])
            assert (wins > 0).all(), (case, np.nonzero(wins == 0)[0][:10])


def test_form_cases_reach_the_branches_their_table_claims():
    """The launch selection of csrc/kmeans.hip restated: tiles of 32 centroids, KT in {1, 2, 4, 8} by the tile count, passes of KT tiles, chunks of 64 columns, the
    LDS histogram up to 1024 clusters, row chunks of 4096 on the unfused route, one-hot chunks of 2^24 / kp rows in the update."""
    import test_gpu_kmeans_forms as forms
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "kmeans.hip")).read()
    assert "constexpr int HIST = 1024;" in src and "return n < 4096 ? n : 4096;" in src and "(1ll << 24) / kp" in src
    assert "if (g.T == 1) SSV_KM(1); else if (g.T == 2) SSV_KM(2); else if (g.T <= 4) SSV_KM(4); else SSV_KM(8);" in src
    seen = set()
    for n, d, k, _ in ko.FORM_CASES:
        tiles = -(-k // 32)
        kt = 1 if tiles == 1 else 2 if tiles == 2 else 4 if tiles <= 4 else 8
        seen.add(("kt", kt))
        seen.add(("ragged block", tiles % kt != 0))
        seen.add(("passes > 1 and padded", tiles > kt and k % 32 != 0))
        seen.add(("chunks", min(-(-d // 64), 3)))
        seen.add(("hist", k <= 1024))
        seen.add(("row chunks", -(-n // 4096) > 1))
        seen.add(("onehot chunks", min(-(-n // max(1, min(n, (1 << 24) // ((k + 3) & ~3)))), 3)))
    for want in [("kt", 1), ("kt", 2), ("kt", 4), ("kt", 8), ("ragged block", True), ("passes > 1 and padded", True), ("chunks", 1), ("chunks", 2), ("chunks", 3),
                 ("hist", True), ("hist", False), ("row chunks", True), ("onehot chunks", 3)]:
        assert want in seen, want
    assert {k for _, _, k, _ in ko.FORM_CASES} >= {250, 500, 1000, 1024, 1025}
    assert max(d for _, d, _, _ in ko.FORM_CASES) == forms.MAX_D == int(re.search(r"#define SSV_KMEANS_MAX_D\s+(\d+)", open(os.path.join(ROOT, "include", "ssv_hip.h")).read()).group(1))


def test_case_table_covers_every_documented_branch():
    """Every branch label of the docstring of tests/test_gpu_kmeans_forms.py is targeted by a test there, no test names an unknown label, the FORM_CASES rows of
    the table are the oracle's, and the accuracy bound respects its caps."""
    import math
    import test_gpu_kmeans_forms as forms
    doc = forms.documented_labels()
    assert len(doc) >= 30
    used = {b for labels in forms.TARGETS.values() for b in labels.split()}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    tests = {name for name in dir(forms) if name.startswith("test_")}
    assert set(forms.TARGETS) == tests, sorted(set(forms.TARGETS) ^ tests)
    assert all(doc[b] in ("ssv_kmeans_assign", "ssv_kmeans_update", "ssv_cluster_votes") for b in doc)
    rows = forms.documented_form_cases()
    assert rows == {i: c for i, c in enumerate(ko.FORM_CASES)}
    assert 1.0 <= forms.FACTOR <= 8.0 and math.log2(forms.FACTOR).is_integer() and 0.0 <= forms.FLOOR <= 16 * 2.0 ** -24


def test_the_accuracy_bound_is_what_the_committed_report_implies():
    """FACTOR = the worst measured ratio of profiles/kmeans_pirl_forms_report.json rounded up to the next power of two, never above 8; FLOOR as measured under."""
    import json
    import forms_report as fr
    import test_gpu_kmeans_forms as forms
    fam = json.load(open(os.path.join(ROOT, "profiles", "kmeans_pirl_forms_report.json")))["families"]["kmeans.dist"]
    worst = max(fam["worst_e_ratio"], fam["worst_m_ratio"])
    assert worst <= 8.0 and fam["FLOOR"] == forms.FLOOR and forms.FACTOR == fr.next_pow2(worst) == fam["FACTOR"]


def test_the_distance_reference_is_well_conditioned():
    """ref32 (tests/kmeans_oracle.py::dist_at in float32) within 1e-3 of ref64 (e and m) at the fp64 labels of every form case and set; the reference is
    identically zero - the relative errors undefined - only where tests/test_gpu_kmeans_forms.py says so (n = k = 1: the row is its own centroid)."""
    import test_gpu_kmeans_forms as forms
    zero = set()
    for index in range(len(ko.FORM_CASES)):
        x, sets = ko.form_case(index)
        for which, c in enumerate(sets):
            labels = ko.assign(x, c)[0]
            r64, r32 = ko.dist_at(x, c, labels, np.float64), ko.dist_at(x, c, labels, np.float32)
            assert r64.dtype == np.float64 and r32.dtype == np.float32 and np.isfinite(r64).all()
            if not np.abs(r64).max() > 0:
                zero.add(index)
                continue
            e, m = forms.errors(r32, r64)
            assert e <= 1e-3 and m <= 1e-3, (ko.FORM_CASES[index], which, e, m)
    assert zero == set(forms.ZERO_REFERENCE)
