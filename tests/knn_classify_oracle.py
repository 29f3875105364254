"""fp64 numpy restatement of the weighted kNN classifier (utils/eval_utils.py::knn_classify over csrc/knnclassify.hip) and the seeded inputs its tests share.

search: S = Q B^T in fp64, a STABLE sort of -S per row (similarity descending, exact ties to the lower index), a NaN score behind every number and NaNs among
themselves by index.  vote: score[c] = sum over the neighbours labelled c of exp((sim - sim[:, 0]) / T), classes by score descending, ties to the lower class.
Everything here is float64; the inputs are float32 values (what the GPU sees), widened.  Inputs are drawn on the CPU from fixed seeds."""
import functools

import numpy as np
import torch

T_DEFAULT = 0.07
EXCUSE = 2.0 ** -14                 # tau_i = EXCUSE * |q_i| * max_j |b_j|: the k-means tolerance of DESIGN 7.6 applied to the product term alone
MU = 2.0 ** -13                     # relative margin between the two best class scores under which an fp32 vote may pick the other one: <= 1024 positive fp32
                                    # additions (<= 2^-14) and the rounding of an exponent argument of at most 2 / 0.07 (~ 2^-18), for each of the two scores
MAX_EXCUSED = 0.01
# (m, n, d, C): the blob shapes.  d = 36 has no bf16-piece kernel (fp32-MFMA route); d = 64 runs once under each arithmetic
BLOB_SHAPES = ((300, 1000, 64, 10), (257, 1500, 36, 100))
INT_SHAPE = (300, 1000, 64, 10)     # features uniform in {-2 .. 2}: every product is exact in both arithmetics
INT_T = 4.0
KS = (1, 20, 200)                   # and k = n, per test


def inv_temp32(temperature):
    """1 / T as the C ABI's float argument carries it."""
    return float(np.float32(1.0 / float(temperature)))


@functools.lru_cache(maxsize=None)
def blobs(index, seed=0):
    """(train [n, d] fp32, train labels [n], test [m, d] fp32, test labels [m]): C Gaussian class centres in d dimensions, noise 0.3 sqrt(d), rows of unit length."""
    m, n, d, c = BLOB_SHAPES[index]
    g = torch.Generator().manual_seed(1000 + 17 * index + seed)
    centres = torch.randn(c, d, generator=g, dtype=torch.float64)
    out = []
    for rows in (n, m):
        y = torch.randint(0, c, (rows,), generator=g)
        x = centres[y] + 0.3 * d ** 0.5 * torch.randn(rows, d, generator=g, dtype=torch.float64)
        x = x / x.norm(dim=1, keepdim=True)
        out += [x.float().numpy(), y.numpy()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def integers(seed=8):
    """The integer family: features uniform in {-2 .. 2}, not normalised; labels uniform in [0, C).  The default seed is one at which no query has tied (or
    nearly tied: relative margin 6e-3 at least) class scores at T = 4 for k in {1, 20, 200, n} - tests/test_knn_classify_cpu.py checks it."""
    m, n, d, c = INT_SHAPE
    g = torch.Generator().manual_seed(2000 + seed)
    draw = lambda rows: torch.randint(-2, 3, (rows, d), generator=g).float().numpy()
    bank, queries = draw(n), draw(m)
    return bank, torch.randint(0, c, (n,), generator=g).numpy(), queries, torch.randint(0, c, (m,), generator=g).numpy()


def similarities(queries, bank):
    with np.errstate(invalid="ignore"):
        return np.asarray(queries, np.float64) @ np.asarray(bank, np.float64).T


def order(s):
    """[m, n] int64: per row of s the column indices by value descending, ties to the lower index, NaN last (by index)."""
    key = np.where(np.isnan(s), np.inf, -(s + 0.0))                # -0 and +0 tie; a NaN behind +inf (a score of -inf keys as +inf too, but sorts before: see below)
    nan = np.isnan(s)
    # two stable keys: numbers before NaNs, then the value
    o = np.argsort(key, axis=1, kind="stable")
    rows = np.arange(s.shape[0])[:, None]
    return np.take_along_axis(o, np.argsort(nan[rows, o], axis=1, kind="stable"), axis=1)


def search(queries, bank, k):
    """(sim [m, k] fp64, idx [m, k] int64) under the search's order rule."""
    s = similarities(queries, bank)
    idx = order(s)[:, :k]
    return np.take_along_axis(s, idx, axis=1), idx


def vote_scores(sim, idx, bank_labels, num_classes, inv_temp):
    """[m, C] fp64: score[c] = sum_{r: label(idx_r) = c} exp((sim_r - sim_0) * inv_temp); an entry with an index or label out of range or a NaN sim is not counted."""
    sim, idx, lab = np.asarray(sim, np.float64), np.asarray(idx, np.int64), np.asarray(bank_labels, np.int64)
    m, k = sim.shape
    ok = (idx >= 0) & (idx < lab.shape[0])
    l = np.where(ok, lab[np.clip(idx, 0, lab.shape[0] - 1)], -1)
    ok &= (l >= 0) & (l < num_classes) & ~np.isnan(sim)
    with np.errstate(invalid="ignore"):
        w = np.where(ok, np.exp((sim - sim[:, :1]) * inv_temp), 0.0)
    scores = np.zeros((m, num_classes))
    np.add.at(scores, (np.repeat(np.arange(m), k), np.where(ok, l, 0).reshape(-1)), w.reshape(-1))
    return scores


def vote_scores_torch(sim, idx, bank_labels, num_classes, inv_temp, dtype):
    """The same lines in torch at ``dtype`` on the CPU, summed in rank order (ref32 of rule (a) of tests/test_gpu_loss_kernels.py with dtype float32)."""
    sim = torch.as_tensor(np.asarray(sim)).to(dtype)
    idx, lab = torch.as_tensor(np.asarray(idx, np.int64)), torch.as_tensor(np.asarray(bank_labels, np.int64))
    w = torch.exp((sim - sim[:, :1]) * torch.tensor(inv_temp, dtype=dtype))
    l = lab[idx]
    scores = torch.zeros(sim.shape[0], num_classes, dtype=dtype)
    for r in range(sim.shape[1]):                                   # rank order
        scores.scatter_add_(1, l[:, r:r + 1], w[:, r:r + 1])
    return scores


def top_classes(scores, topn):
    """[m, topn] int64: classes by score descending, ties to the lower class."""
    return np.argsort(-np.asarray(scores, np.float64), axis=1, kind="stable")[:, :topn]


def vote(sim, idx, bank_labels, num_classes, temperature, topn=1):
    scores = vote_scores(sim, idx, bank_labels, num_classes, inv_temp32(temperature))
    return top_classes(scores, topn), scores


def relative_margin(scores):
    """[m] fp64: (best - second best) / best of the class scores (inf with one class)."""
    if scores.shape[1] < 2:
        return np.full(scores.shape[0], np.inf)
    two = -np.partition(-scores, 1, axis=1)[:, :2]
    return (two[:, 0] - two[:, 1]) / np.maximum(two[:, 0], 1e-300)


def classify(train, train_labels, test, test_labels, k, temperature, num_classes, topn=None):
    """{"top1", "top5", "pred", "scores", "sim", "idx"} in fp64 (the features as given: normalise them first if they are not)."""
    sim, idx = search(test, train, min(k, train.shape[0]))
    topn = min(5, num_classes) if topn is None else topn
    pred, scores = vote(sim, idx, train_labels, num_classes, temperature, topn)
    hit = pred == np.asarray(test_labels)[:, None]
    return {"top1": float(hit[:, 0].mean()), "top5": float(hit.any(1).mean()) if num_classes >= 5 else None, "pred": pred, "scores": scores, "sim": sim, "idx": idx}


def tau(queries, bank):
    """[m] fp64: tau_i = 2^-14 |q_i| max_j |b_j|."""
    q, b = np.asarray(queries, np.float64), np.asarray(bank, np.float64)
    return EXCUSE * np.sqrt((q * q).sum(1)) * np.sqrt((b * b).sum(1)).max()


def straddling_ties(s, k):
    """[m] bool: the k-th best value of the row also occurs behind the k-th place (k < n), so the tie rule decides who is returned."""
    srt = -np.sort(-s, axis=1)
    return srt[:, k - 1] == srt[:, k] if k < s.shape[1] else np.zeros(s.shape[0], bool)
