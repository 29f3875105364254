"""fp64 numpy restatement of the kNN label agreement (ssv_knn_label_agreement_arith, csrc/evalknn.hip), neighbour by neighbour, and the seeded inputs and labellings
its tests share (tests/test_knn_agreement_cpu.py, tests/test_gpu_knn_agreement.py).

Neighbour lists.  S = Z Z^T in fp64 from the fp32 values; each row ordered by knn_classify_oracle.order (value descending, ties to the lower index, NaN last);
rank 0 is dropped blindly (normally the query itself, but not always) and ranks 1 .. k are kept.  A NaN score never enters a list (the kernel's documented
rule): a row holding a NaN is nobody's neighbour, and a query whose OWN row holds a NaN has every score NaN and contributes NOTHING to the count.  Features
containing +-inf are out of scope: the fused and the unfused route treat a score of -inf differently (the one's empty slots are -inf themselves), and no
caller produces one.

Labellings.  One count under one labelling hides most wrong neighbours; labelings() is a fixed family under which a single wrong neighbour always shows: all
equal (the count is the number of neighbours returned), all distinct (0), the bit planes (i >> b) & 1 of the index (two different indices differ in some bit,
so replacing one neighbour by another at one query moves the count of that plane by one) and 16 seeded random labellings.

Windows for fp32 features.  tau_q = 16 * 2^-24 * max_j sum_c |z_qc| |z_jc|: rule (a) of tests/test_gpu_conv_forms.py with its TAU["fwd"] - the Gram product is
that forward kernel, and the fused kernel is the same six-piece product.  With t the fp64 (k+1)-th best score of the row, the rows other than the dropped hit
split into the certain set A (s > t + 2 tau), the uncertain set U (|s - t| <= 2 tau) and the rest; the query contributes between
match(A) + max(0, k - |A| - nonmatch(U)) and match(A) + min(k - |A|, match(U)).  Everything here is GPU-free; nothing is measured from a kernel."""
import functools

import numpy as np
import torch

import knn_classify_oracle as kc

U24 = 2.0 ** -24
TAU_FWD = 16.0                      # TAU["fwd"] of tests/test_gpu_conv_forms.py (tests/test_knn_agreement_cpu.py checks that they agree)
MAX_EXCUSED = kc.MAX_EXCUSED
MAX_WIDTH = 2                       # hi - lo of a window, per labelling
ROW_CHUNK = 2048                    # rows of S formed at a time


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def small_ints(n, d, seed, low=-2, high=2):
    """Features uniform in {low .. high}: every product and every sum is exact in both arithmetics, and the rows are full of ties."""
    return torch.randint(low, high + 1, (n, d), generator=_gen(3000 + seed)).float().numpy()


def two_piece_ints(n, seed, d=32):
    """Integers in {-300 .. 300}: exact products, sums below 2^24 in fp32 up to d = 96, and values that need TWO bf16 pieces (the odd ones above 256: 7 % of the
    values, some in nearly every row) - the cross terms of the six-piece product matter."""
    return small_ints(n, d, 100 + seed, -300, 300)


def blob_features(n, d, seed, classes=10):
    """knn_classify_oracle.blobs' generator at any shape: Gaussian class centres, noise 0.3 sqrt(d), rows of unit length."""
    g = _gen(4000 + seed)
    centres = torch.randn(classes, d, generator=g, dtype=torch.float64)
    y = torch.randint(0, classes, (n,), generator=g)
    x = centres[y] + 0.3 * d ** 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().numpy()


def relu_features(n, d, seed, classes=10):
    """What a backbone hands over: post-ReLU activations around a common positive mean (relu(1 + class centre / 2 + noise / 2)), not normalised, row scales
    uniform in [0.5, 1.5] - the rows are much alike and the long ones win, so the best hit is mostly NOT the query itself."""
    g = _gen(5000 + seed)
    centres = torch.randn(classes, d, generator=g, dtype=torch.float64)
    y = torch.randint(0, classes, (n,), generator=g)
    x = torch.relu(1.0 + 0.5 * centres[y] + 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64))
    return (x * (0.5 + torch.rand(n, 1, generator=g, dtype=torch.float64))).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------- labellings
RANDOM_CLASSES = (2, 2, 2, 2, 3, 5, 10, None)      # None: n // 2 classes; each twice


@functools.lru_cache(maxsize=None)
def labelings(n, seed=0):
    """((name, int32 [n]), ...): all equal, all distinct, every bit plane of the index below n, 16 seeded random labellings."""
    out = [("equal", np.zeros(n, np.int32)), ("distinct", np.arange(n, dtype=np.int32))]
    b = 0
    while (1 << b) < n:
        out.append((f"bit{b}", ((np.arange(n) >> b) & 1).astype(np.int32)))
        b += 1
    g = _gen(6000 + seed)
    for rep in range(2):
        for c in RANDOM_CLASSES:
            c = max(n // 2, 1) if c is None else c
            out.append((f"rand{c}.{rep}.{len(out)}", torch.randint(0, c, (n,), generator=g).numpy().astype(np.int32)))
    for _, lab in out:
        lab.setflags(write=False)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------- neighbour lists
def scores(z, r0=0, r1=None):
    """Rows r0 .. r1 of S = Z Z^T in fp64."""
    z = np.asarray(z, np.float32)
    return kc.similarities(z[r0:r1], z)


def top(s, m):
    """The first m columns of knn_classify_oracle.order(s), without sorting whole rows: only the columns at or above the row's m-th best value can reach them."""
    n = s.shape[1]
    if m >= n:
        return kc.order(s)[:, :m]
    key = np.where(np.isnan(s), np.inf, -(s + 0.0))
    kth = np.partition(key, m - 1, axis=1)[:, m - 1]
    out = np.empty((s.shape[0], m), np.int64)
    for r in range(s.shape[0]):
        cand = np.flatnonzero(key[r] <= kth[r])                  # ascending, so the stable order keeps ties at the lower index
        out[r] = cand[kc.order(s[r:r + 1, cand])[0, :m]]
    return out


def lists(z, k):
    """[n, k] int64: ranks 1 .. k of every query; -1 where there is no neighbour (a NaN score never enters: the whole row of a query that holds a NaN)."""
    z = np.asarray(z, np.float32)
    n = z.shape[0]
    assert 1 <= k < n
    idx = np.empty((n, k), np.int64)
    for r0 in range(0, n, ROW_CHUNK):
        s = scores(z, r0, r0 + ROW_CHUNK)
        t = top(s, k + 1)[:, 1:]
        idx[r0:r0 + ROW_CHUNK] = np.where(np.isnan(np.take_along_axis(s, t, axis=1)), -1, t)
    return idx


def count(idx, lab):
    """Label matches over a padded index table (-1: no entry)."""
    lab = np.asarray(lab)
    return int(((lab[np.maximum(idx, 0)] == lab[:, None]) & (idx >= 0)).sum())


def expected(z, lab, k, idx=None):
    """The exact count from the lists."""
    return count(lists(z, k) if idx is None else idx, lab)


# ---------------------------------------------------------------------------------------------------------------------- windows
class Margins:
    """Per query: the certain set A and the uncertain set U as padded index tables, tau, and whether the dropped hit itself is ambiguous."""

    def __init__(self, a, u, tau, ambiguous, k):
        self.a, self.u, self.tau, self.ambiguous, self.k = a, u, tau, ambiguous, k
        self.excused = (u >= 0).sum(1) > 1

    @property
    def excused_share(self):
        return float(self.excused.mean())


def _padded(rows):
    width = max(1, max(len(r) for r in rows))
    out = np.full((len(rows), width), -1, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def margins(z, k):
    z = np.asarray(z, np.float32)
    n = z.shape[0]
    assert 1 <= k < n and np.isfinite(z).all()
    za = np.abs(z.astype(np.float64))
    a_rows, u_rows, taus, amb = [], [], [], []
    for r0 in range(0, n, ROW_CHUNK):
        s = scores(z, r0, r0 + ROW_CHUNK)
        tau = TAU_FWD * U24 * (za[r0:r0 + ROW_CHUNK] @ za.T).max(1)
        t = top(s, k + 1)
        rows = np.arange(s.shape[0])
        best, second, kth = s[rows, t[:, 0]], s[rows, t[:, 1]], s[rows, t[:, k]]
        amb.append(best - second <= 2 * tau)
        other = np.ones(s.shape, bool)
        other[rows, t[:, 0]] = False
        certain = other & (s > (kth + 2 * tau)[:, None])
        unsure = other & (np.abs(s - kth[:, None]) <= 2 * tau[:, None])
        a_rows += [np.flatnonzero(r) for r in certain]
        u_rows += [np.flatnonzero(r) for r in unsure]
        taus.append(tau)
    return Margins(_padded(a_rows), _padded(u_rows), np.concatenate(taus), np.concatenate(amb), k)


def window(z, lab, k, m=None):
    """(lo, hi, excused_share): the counts any search whose scores are within tau_q of fp64 can return."""
    m = margins(z, k) if m is None else m
    lab = np.asarray(lab)
    same = lambda t: (lab[np.maximum(t, 0)] == lab[:, None]) & (t >= 0)
    size_a, size_u = (m.a >= 0).sum(1), (m.u >= 0).sum(1)
    match_a, match_u = same(m.a).sum(1), same(m.u).sum(1)
    free = k - size_a
    assert (free >= 0).all()
    lo = match_a + np.maximum(0, free - (size_u - match_u))
    hi = match_a + np.minimum(free, match_u)
    return int(lo.sum()), int(hi.sum()), m.excused_share
