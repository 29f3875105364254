"""fp64 numpy restatement of the product's Lloyd k-means (utils/eval_utils.py::kmeans over csrc/kmeans.hip) and the seeded inputs the k-means tests share.

assign: arg-min of the squared distance, exact ties to the lowest index (numpy's argmin returns the first minimum); update: mean of the members, a cluster
without members keeps its centroid; objective: sum of the squared distances to the assigned centroids; the same initial rows and the same redo rule as the
product.  Everything here is float64; the inputs are float32 values (what the GPU sees), widened."""
import functools

import numpy as np
import torch

# (n, d, k, spread): the assignment cases of tests/test_gpu_kmeans.py; tests/test_kmeans_cpu.py proves in fp64 that at most 1 % of their rows are near-ties
ASSIGN_CASES = ((389, 32, 10, 1.0), (1000, 96, 33, 2.0), (2048, 512, 100, 3.0), (777, 2048, 10, 4.0), (4096, 128, 256, 50.0),
                (130, 20, 3, 1.0),          # d is not a multiple of 4
                (64, 32, 1, 1.0))           # k = 1, n below one row block
# the sizes at which the code takes another path, held to the same checks
PATH_CASES = ((5000, 16, 4096, 1.0),        # k > 1024: counts go straight to the global counters, 16 passes of 256 centroids in the fused kernel, two one-hot chunks in the update
              (4226, 24, 40, 2.0))          # n > 4096: two row chunks of the unfused product, the last one short
ALL_CASES = ASSIGN_CASES + PATH_CASES
# the launch forms of tests/test_gpu_kmeans_forms.py (its docstring says which branch each one reaches); tests/test_kmeans_cpu.py proves in fp64 that they stay under
# the same near-tie cap and that every centroid of every set wins a row
FORM_CASES = ((257, 64, 1, 1.0), (300, 32, 31, 1.0), (300, 32, 32, 1.0), (400, 64, 64, 2.0), (500, 68, 70, 2.0), (700, 60, 130, 2.0), (900, 128, 200, 2.0),
              (1500, 128, 250, 2.0), (1200, 16, 257, 1.0), (1500, 48, 300, 2.0), (2000, 128, 500, 3.0), (3000, 128, 1000, 3.0), (1100, 16, 1024, 1.0),
              (1100, 16, 1025, 1.0), (130, 8192, 3, 4.0), (200, 4096, 40, 4.0), (129, 4, 5, 1.0), (127, 36, 9, 1.0), (128, 36, 9, 1.0), (4097, 16, 7, 1.0),
              (8195, 16, 4096, 1.0), (1, 4, 1, 1.0))
EXCUSE = 2.0 ** -14                         # tau_i = EXCUSE * (|x_i|^2 + max_j |c_j|^2): the margin under which an fp32 assignment may differ from the fp64 one
MAX_EXCUSED = 0.01


def blobs(seed, n, d, k, spread):
    """x [n, d] float32 = centre[label] + spread * noise, labels [n] int64: centres randn(k, d), uniform random labels."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(k, d, generator=g)
    labels = torch.randint(0, k, (n,), generator=g)
    x = centres[labels] + spread * torch.randn(n, d, generator=g)
    return x.float().numpy(), labels.numpy()


def init_rows(seed, n, k):
    """The rows a run seeded `seed` starts from (the product's draw)."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].numpy()


def sqdist(x, c):
    """[n, k] squared distances in fp64 (clamped at 0)."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.maximum((x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), 0.0)


def assign(x, c):
    """(labels [n] int64, dist [n] fp64): nearest centroid, exact ties to the lowest index."""
    dm = sqdist(x, c)
    labels = dm.argmin(1)
    return labels, dm[np.arange(dm.shape[0]), labels]


def update(x, labels, c):
    """New centroids [k, d] fp64: the mean of each cluster's members; a cluster without members keeps its row of c."""
    x = np.asarray(x, np.float64)
    out = np.array(c, np.float64, copy=True)
    for j in range(out.shape[0]):
        members = x[labels == j]
        if members.shape[0]:
            out[j] = members.mean(0)
    return out


def objective(x, c, labels=None):
    return float(assign(x, c)[1].sum()) if labels is None else float(sqdist(x, c)[np.arange(len(labels)), labels].sum())


def lloyd(x, k, niter, seed):
    """One run: {"centroids", "labels", "objective", "objectives"} with objectives[i] the objective of iteration i's assignment."""
    x = np.asarray(x, np.float64)
    c = x[init_rows(seed, x.shape[0], k)].copy()
    trace = []
    for _ in range(niter):
        labels, dist = assign(x, c)
        trace.append(float(dist.sum()))
        c = update(x, labels, c)
    labels, dist = assign(x, c)
    return {"centroids": c, "labels": labels, "objective": float(dist.sum()), "objectives": trace}


def kmeans(x, k, niter=25, nredo=1, seed=1234):
    """The redo rule: run r starts from init_rows(seed + r); the lowest final objective wins, the lower r on a tie."""
    best = None
    for r in range(nredo):
        run = lloyd(x, k, niter, seed + r)
        run["redo"] = r
        if best is None or run["objective"] < best["objective"]:
            best = run
    return best


def margins(x, c):
    """Per row, in fp64: (best squared distance, margin = second best - best (inf for k = 1), tau_i)."""
    dm = sqdist(x, c)
    if dm.shape[1] > 1:
        two = np.partition(dm, 1, axis=1)[:, :2]
        best, margin = two[:, 0], two[:, 1] - two[:, 0]
    else:
        best, margin = dm[:, 0], np.full(dm.shape[0], np.inf)
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    tau = EXCUSE * ((x64 * x64).sum(1) + (c64 * c64).sum(1).max())
    return best, margin, tau


@functools.lru_cache(maxsize=None)
def assign_case(index):
    """(x float32 [n, d], [c0, c1, c2] float32): the case's blobs and its three centroid sets - the initial rows, then one and two oracle updates, rounded to
    float32 (the values both the GPU and the fp64 reference are given)."""
    return _case(ALL_CASES[index], 100 + index, 200 + index)


@functools.lru_cache(maxsize=None)
def form_case(index):
    """assign_case over FORM_CASES: blobs(300 + index, ...), init_rows(400 + index, ...)."""
    return _case(FORM_CASES[index], 300 + index, 400 + index)


def _case(case, blob_seed, init_seed):
    n, d, k, spread = case
    x, _ = blobs(blob_seed, n, d, k, spread)
    c = x[init_rows(init_seed, n, k)].astype(np.float64)
    sets = [c.astype(np.float32)]
    for _ in range(2):
        c = update(x, assign(x, sets[-1])[0], sets[-1])
        sets.append(c.astype(np.float32))
    return x, sets


def dist_at(x, c, labels, dtype):
    """[n] squared distances to the centroids `labels` names, |x|^2 + |c_l|^2 - 2 x . c_l, every line in `dtype`: the reference of the accuracy rule of
    tests/test_gpu_kmeans_forms.py in float64 and the SAME lines in float32."""
    x, cl = np.asarray(x, dtype), np.asarray(c, dtype)[labels]
    return (x * x).sum(1) + (cl * cl).sum(1) - dtype(2.0) * (x * cl).sum(1)


def update_bound(x, labels, k):
    """[k, d] element-wise bound on |fp32 mean - fp64 mean| of each cluster: (m + 2) * 2^-24 * sum_{i in c} |x_i| / m (m - 1 fp32 additions and one division);
    0 for a cluster without members (its centroid must not move)."""
    x = np.abs(np.asarray(x, np.float64))
    out = np.zeros((k, x.shape[1]))
    for j in range(k):
        members = x[labels == j]
        m = members.shape[0]
        if m:
            out[j] = (m + 2) * 2.0 ** -24 * members.sum(0) / m
    return out
