"""GPU: k-means (csrc/kmeans.hip through ops / utils.eval_utils) and the Hungarian-matched cluster accuracy against the fp64 oracle of
tests/kmeans_oracle.py, in BOTH arithmetics (bf16x3: the search fused into the X C^T product; f32: GEMM through the workspace + one wavefront per row).

Assignment.  A row is EXCUSED when its fp64 margin (second best minus best squared distance) is below tau_i = 2^-14 (|x_i|^2 + max_j |c_j|^2); every other row
must carry the fp64 label exactly, an excused row a label whose fp64 distance is within tau_i of the best, and at most 1 % of the rows may be excused
(tests/test_kmeans_cpu.py shows in fp64 that the inputs stay under that cap: at most 0.4 %).  |dist - dist64| <= tau_i, |objective - sum dist64| <= sum tau_i,
counts == bincount(labels).
Update.  Per cluster of m members |got - want| <= (m + 2) 2^-24 sum |x_i| / m element-wise (m - 1 fp32 additions in whatever fixed order, one division); a cluster
without members keeps its centroid bit for bit."""
import os

import numpy as np
import pytest
import torch
import yaml

import kmeans_oracle as ko

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITHMETICS = ("bf16x3", "f32")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check_assignment(x, c, labels, dist, counts, objective):
    """The assignment contract of the module docstring for one (x, centroids) pair; tensors from ops.kmeans_assign."""
    n, k = x.shape[0], c.shape[0]
    labels, dist, counts = labels.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.float64), counts.cpu().numpy().astype(np.int64)
    assert labels.min() >= 0 and labels.max() < k
    dm = ko.sqdist(x, c)
    best, margin, tau = ko.margins(x, c)
    want = dm.argmin(1)
    excused = margin < tau
    share = float(excused.mean())
    print(f"n={n} d={x.shape[1]} k={k}: excused {share:.4%}, label mismatches {int((labels != want).sum())}, max |dist err| / tau {float((np.abs(dist - best) / tau).max()):.3e}, "
          f"|obj err| / sum tau {abs(float(objective) - best.sum()) / tau.sum():.3e}")
    assert share <= ko.MAX_EXCUSED, share
    assert np.array_equal(labels[~excused], want[~excused]), np.nonzero((labels != want) & ~excused)[0][:10]
    got_d64 = dm[np.arange(n), labels]
    assert (got_d64[excused] - best[excused] <= tau[excused]).all()
    assert (np.abs(dist - best) <= tau).all(), float((np.abs(dist - best) / tau).max())
    assert abs(float(objective) - best.sum()) <= tau.sum()
    assert np.array_equal(counts, np.bincount(labels, minlength=k)) and counts.sum() == n


@pytest.mark.parametrize("arith", ARITHMETICS)
@pytest.mark.parametrize("index", range(len(ko.ALL_CASES)))
def test_assignment_against_fp64(index, arith):
    from ssv_amd import ops
    x, sets = ko.assign_case(index)
    xd = _dev(x)
    with ops.arithmetic(arith):
        for c in sets:
            _check_assignment(x, c, *ops.kmeans_assign(xd, _dev(c)))


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_ties_go_to_the_lowest_index(arith):
    from ssv_amd import ops
    x, sets = ko.assign_case(1)                                  # n 1000, d 96, k 33
    rows = ko.init_rows(200 + 1, x.shape[0], 33)
    xd = _dev(x)
    with ops.arithmetic(arith):
        for which, c in enumerate(sets[:2]):
            c = c.copy()
            c[5] = c[2]                                          # bit-identical rows: bit-identical scores, the lower index wins
            labels, dist, counts, _ = ops.kmeans_assign(xd, _dev(c))
            labels, dist = labels.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
            assert not (labels == 5).any() and int(counts[5]) == 0 and (labels == 2).any()
            if which == 0:                                       # the initial centroids ARE rows of x: such a row gets its own centroid (or a lower-indexed copy of it)
                _, _, tau = ko.margins(x, c)
                for j, i in enumerate(rows):
                    if j == 5:                                   # its centroid was overwritten by the copy of centroid 2
                        continue
                    assert labels[i] <= j and np.array_equal(c[labels[i]], c[j]), (j, i, labels[i])
                    assert dist[i] <= tau[i]
                assert labels[rows[2]] == 2


@pytest.mark.parametrize("arith", ARITHMETICS)
@pytest.mark.parametrize("index", range(len(ko.ALL_CASES)))
def test_update_against_fp64_on_the_gpus_own_labels(index, arith):
    from ssv_amd import ops
    x, sets = ko.assign_case(index)
    k = sets[0].shape[0]
    xd = _dev(x)
    with ops.arithmetic(arith):
        cd = _dev(sets[0])
        labels, _, counts, _ = ops.kmeans_assign(xd, cd)
        before = cd.clone()
        out = ops.kmeans_update(xd, labels, counts, cd)
    assert out is cd
    lab = labels.cpu().numpy().astype(np.int64)
    want = ko.update(x, lab, sets[0])
    bound = ko.update_bound(x, lab, k)
    err = np.abs(cd.cpu().numpy().astype(np.float64) - want)
    print(f"case {ko.ALL_CASES[index]} {arith}: max err / bound {float((err / np.maximum(bound, 1e-300))[bound > 0].max()):.3e}")
    assert (err <= bound).all(), float((err - bound).max())
    empty = np.bincount(lab, minlength=k) == 0
    assert torch.equal(_bits(cd)[torch.as_tensor(empty)], _bits(before)[torch.as_tensor(empty)])


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_update_keeps_the_centroid_of_an_empty_cluster(arith):
    from ssv_amd import ops
    x, sets = ko.assign_case(0)                                  # n 389, d 32, k 10
    n, k = x.shape[0], 10
    lab = np.arange(n) % k
    lab[(lab == 1) | (lab == 4)] = 0                             # clusters 1 and 4 lose every member
    counts = np.bincount(lab, minlength=k)
    cd = _dev(sets[0])
    before = cd.clone()
    with ops.arithmetic(arith):
        ops.kmeans_update(_dev(x), _dev(lab, torch.int32), _dev(counts, torch.int32), cd)
    assert torch.equal(_bits(cd)[[1, 4]], _bits(before)[[1, 4]])
    err = np.abs(cd.cpu().numpy().astype(np.float64) - ko.update(x, lab, sets[0]))
    assert (err <= ko.update_bound(x, lab, k)).all()
    assert not torch.equal(_bits(cd)[0], _bits(before)[0])


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_equal_inputs_give_equal_bits(arith):
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    x, sets = ko.assign_case(2)                                  # n 2048, d 512, k 100: 16 row blocks
    xd = _dev(x)
    with ops.arithmetic(arith):
        a, b = ops.kmeans_assign(xd, _dev(sets[1])), ops.kmeans_assign(xd, _dev(sets[1]))
        for u, v in zip(a, b):
            assert torch.equal(_bits(u), _bits(v))
        c1, c2 = _dev(sets[1]), _dev(sets[1])
        ops.kmeans_update(xd, a[0], a[2], c1)
        ops.kmeans_update(xd, a[0], a[2], c2)
        assert torch.equal(_bits(c1), _bits(c2))
        xs, _ = ko.blobs(7, 1000, 64, 10, 0.2)
        r1, r2 = (eval_utils.kmeans(xs, 10, niter=5, nredo=2) for _ in range(2))
    assert torch.equal(r1["labels"], r2["labels"]) and torch.equal(_bits(r1["centroids"]), _bits(r2["centroids"]))
    assert np.float32(r1["objective"]).tobytes() == np.float32(r2["objective"]).tobytes() and r1["objectives"] == r2["objectives"]


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_a_whole_run_against_the_oracle(arith):
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    n, d, k, niter = 1000, 64, 10, 8
    x, _ = ko.blobs(7, n, d, k, 0.2)
    want = ko.kmeans(x, k, niter=niter, nredo=2, seed=1234)
    with ops.arithmetic(arith):
        got = eval_utils.kmeans(x, k, niter=niter, nredo=2, seed=1234)
    assert got["redo"] == want["redo"]
    labels = got["labels"].cpu().numpy().astype(np.int64)
    assert np.array_equal(labels, want["labels"])
    # the returned centroids are the update of the last iteration's assignment; the oracle's labels of that iteration
    x64 = x.astype(np.float64)
    c = x64[ko.init_rows(1234 + want["redo"], n, k)]
    for _ in range(niter):
        last = ko.assign(x, c)[0]
        c = ko.update(x, last, c)
    err = np.abs(got["centroids"].cpu().numpy().astype(np.float64) - want["centroids"])
    assert (err <= ko.update_bound(x, last, k)).all(), float(err.max())
    tau_sum = float(ko.margins(x, want["centroids"])[2].sum())
    trace = got["objectives"] + [got["objective"]]
    assert len(got["objectives"]) == niter
    assert all(b <= a + tau_sum for a, b in zip(trace, trace[1:])), trace
    assert abs(got["objective"] - want["objective"]) <= tau_sum


def test_cluster_votes_against_histogram2d():
    from ssv_amd import ops
    from ssv_amd._lib import SsvError
    rng = np.random.default_rng(5)
    for n, pk, tk in ((5000, 7, 12), (1, 3, 2), (300, 1, 1)):
        pred, tgt = rng.integers(0, pk, n), rng.integers(0, tk, n)
        votes = ops.cluster_votes(_dev(pred, torch.int32), _dev(tgt, torch.int32), pk, tk)
        want = np.histogram2d(pred, tgt, bins=(np.arange(pk + 1), np.arange(tk + 1)))[0]
        assert votes.dtype == torch.int64 and np.array_equal(votes.cpu().numpy(), want.astype(np.int64))
    pred = rng.integers(0, 4, 100)
    pred[17] = 4                                                 # == pred_k
    with pytest.raises(SsvError):
        ops.cluster_votes(_dev(pred, torch.int32), _dev(rng.integers(0, 4, 100), torch.int32), 4, 4)
    with pytest.raises(SsvError):
        ops.cluster_votes(_dev(rng.integers(0, 4, 100), torch.int32), _dev(np.full(100, -1), torch.int32), 4, 4)


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_cluster_accuracy_against_the_oracle_route(arith):
    from oracle import evalknn
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    x, y = evalknn.clustered_features(81, 700, 126, 10, 0.5)
    n = x.shape[0]
    with ops.arithmetic(arith):
        got = eval_utils.compute_cluster_accuracy(x, y)
    run = ko.kmeans(x, 10)
    pairs = eval_utils.hungarian_match(run["labels"], y, 10, 10)
    want = sum(int(((run["labels"] == p) & (y == t)).sum()) for p, t in pairs) / n
    print(f"cluster accuracy {got:.4f}, oracle route {want:.4f}")
    assert abs(got - want) <= 1.0 / n + 1e-12
    # a permuted copy of the true labels through the votes and the matching: exactly 1
    from scipy.optimize import linear_sum_assignment
    perm = np.random.default_rng(3).permutation(10)
    votes = ops.cluster_votes(_dev(perm[y], torch.int32), _dev(y, torch.int32), 10, 10).cpu().numpy()
    rows, cols = linear_sum_assignment(n - votes)
    assert votes[rows, cols].sum() / n == 1.0


def test_refusals():
    from ssv_amd import _lib, ops
    from ssv_amd._lib import SsvError
    x = torch.randn(64, 16, generator=torch.Generator().manual_seed(0))
    xd = x.cuda()
    cd = xd[:4].contiguous()
    lab, cnt = torch.zeros(64, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    with pytest.raises(SsvError):
        ops.kmeans_assign(x, x[:4].contiguous())                 # CPU tensors
    with pytest.raises(SsvError):
        ops.kmeans_update(xd, lab.cpu(), cnt, cd)
    with pytest.raises(SsvError):
        ops.cluster_votes(lab.cpu(), lab.cpu(), 2, 2)
    with pytest.raises(SsvError):
        ops.kmeans_assign(torch.randn(16, 64).cuda().t(), cd)    # a non-contiguous x
    with pytest.raises(SsvError):
        ops.kmeans_assign(xd[:3].contiguous(), cd)               # k > n
    big = torch.zeros(_lib.KMEANS_MAX_K + 8, 4).cuda()
    with pytest.raises(SsvError):
        ops.kmeans_assign(big, big[:_lib.KMEANS_MAX_K + 1].contiguous())      # k above the limit
    with pytest.raises(SsvError):
        ops.kmeans_assign(xd, torch.zeros(4, 12).cuda())         # centroids of another width
    with pytest.raises(SsvError):
        ops.kmeans_update(xd, lab, cnt, torch.zeros(4, 12).cuda())
    # the C ABI itself refuses what the wrapper would have caught (status + ssv_last_error text), before any launch
    lib = _lib.load()
    prep = torch.empty(max(lib.ssv_kmeans_prep_bytes(16, 4), 16), dtype=torch.uint8).cuda()
    out = torch.empty(64, dtype=torch.float32).cuda()
    ws = torch.empty(1 << 20, dtype=torch.uint8).cuda()
    args = lambda n, d, k: (n, d, k, xd.data_ptr(), cd.data_ptr(), prep.data_ptr(), 0, lab.data_ptr(), out.data_ptr(), cnt.data_ptr(), out.data_ptr(), 6,
                            ws.data_ptr(), ws.numel(), _lib.stream())
    for n, d, k in ((3, 16, 4), (64, 16, _lib.KMEANS_MAX_K + 1), (64, 18, 4), (64, _lib.KMEANS_MAX_D + 4, 4), (-1, 16, 4)):
        assert lib.ssv_kmeans_assign(*args(n, d, k)) == -1 and b"ssv_kmeans_assign" in lib.ssv_last_error()
    assert lib.ssv_kmeans_workspace_bytes(3, 16, 4, 6) == 0 and lib.ssv_kmeans_prep_bytes(16, _lib.KMEANS_MAX_K + 1) == 0
    with pytest.raises(ValueError):
        from ssv_amd.utils import eval_utils
        eval_utils.kmeans(x.numpy(), 65)


def test_main_cluster_eval_from_a_checkpoint(tmp_path, monkeypatch):
    """`-t cluster_eval -l <dir>` on a one-epoch synthetic resnet18 checkpoint: returns the model and logs the accuracy."""
    from ssv_amd import main as cli
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "simclr.yaml")))
    cfg["epochs"], cfg["eval_every"] = 1, 1
    cfg["data"]["batch_size"] = 32
    cfg["data"]["synthetic"] = {"num_train": 64, "num_test": 48, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"]["epochs"] = 1
    cfg["cluster_eval"] = {"niter": 6, "nredo": 2, "seed": 3}
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    cli.main(["-c", str(path), "-a", "simclr", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "simclr" / "resnet18" / "run"
    assert (out / "best_model.pt").exists()
    model = cli.main(["-c", str(path), "-a", "simclr", "-m", "resnet18", "-t", "cluster_eval", "-o", "cluster", "-l", str(out)])
    assert model is not None and hasattr(model, "cluster_validate")
    log = (tmp_path / "outputs" / "simclr" / "resnet18" / "cluster" / "trainlogs.txt").read_text()
    lines = [ln for ln in log.splitlines() if "Test cluster accuracy:" in ln]
    assert len(lines) == 1
    acc = float(lines[0].split("Test cluster accuracy:")[1])
    assert 0.0 <= acc <= 1.0
