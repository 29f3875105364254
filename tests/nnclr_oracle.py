"""fp64 restatement of NNCLR's two pieces (Dwibedi et al., ICCV 2021) and the seeded inputs tests/test_nnclr_cpu.py and tests/test_gpu_nnclr.py share.

lookup (csrc/nnlookup.hip: ssv_nn_lookup): S = Q B^T in float64 on the float32 values the GPU sees; idx = the first arg-max of every row (exact ties to the lowest
index: numpy's argmax), the margin between the best and the second best score, and tau_i = 2^-14 |q_i| max_j |b_j| - EXCUSE and the cap MAX_EXCUSED on the share
of rows whose margin lies below it are those of tests/knn_classify_oracle.py.

loss (utils/losses.py: NnclrLoss), parameterised by dtype (float64 is the reference, the SAME lines in float32 give ref32).  With a = inv_T * bank[idx] (one fp32
multiply - the lookup's output, so the same fp32 values in every dtype), p_hat = p / max(|p|, eps):
    l(a, p) = mean_i [ logsumexp_j (a_i . p_hat_j) - a_i . p_hat_i ]
    loss    = 1/2 (l(a1, p2) + l(a2, p1))           a1 = neighbours of z1, a2 = neighbours of z2
Only the row-direction cross-entropy of the paper's eq. 3.  The neighbour indices are an INPUT of these lines (the lookup is judged on its own)."""
import functools
from collections import namedtuple

import numpy as np
import torch

from knn_classify_oracle import EXCUSE, MAX_EXCUSED  # noqa: F401

L2_EPS = 1e-12

# (m, n, d): the smallest shapes that reach each path of the lookup
LOOKUP_SHAPES = ((8, 16, 32),            # one tile of everything
                 (130, 1000, 96),        # two ragged row blocks, a ragged bank tile, d no multiple of 64
                 (300, 4100, 256),       # more queries than one resident block (256), several bank slices
                 (64, 70000, 128))       # many slices to fold; two parts of the bank on the unfused route
KINDS = ("gauss", "clustered")
LookupCase = namedtuple("LookupCase", "m n d kind")
LOOKUP_CASES = {f"{m}x{n}x{d}-{k}": LookupCase(m, n, d, k) for m, n, d in LOOKUP_SHAPES for k in KINDS}
# case id -> seed offset, where the default (0) puts the case over the near-tie cap: with 64 queries ONE row within tau of a tie is 1.6 % (offsets 0 and 1 of the
# gauss case, 0 of the clustered one have such a row; the ones taken have none)
SEEDS = {"64x70000x128-gauss": 2, "64x70000x128-clustered": 1}

# ---- the launch forms (tests/test_gpu_nn_lookup_forms.py): (m, n, d), the smallest shape that reaches each form of csrc/nnlookup.hip the table above leaves out
FORM_BIG_N = (1 << 21) + 600                                             # above SSV_NN_LOOKUP_SLICE * SSV_NN_LOOKUP_MAX_SLICES rows a slice doubles
FORM_LOOKUP_SHAPES = ((96, 600, 32),          # three query tiles: nn_fused_k<4> with the fourth tile repeated and unwritten
                      (128, 1299, 96),        # four full tiles, three slices, d % 64 = 32
                      (70, 300, 1024),        # the widest fused width: 16 chunk trips
                      (40, 300, 36),          # d % 32 != 0: unfused in both arithmetics
                      (40, 300, 1056),        # above the fused limit: unfused in both arithmetics
                      (1030, 200, 32),        # 33 tiles: five blocks of 8, the last with one live tile
                      (1030, 200, 36),        # two query chunks on the unfused route
                      (8, FORM_BIG_N, 32))    # L = 1024: a wave's quarter is 256 rows
FORM_LOOKUP_CASES = {f"{m}x{n}x{d}-{k}": LookupCase(m, n, d, k) for m, n, d in FORM_LOOKUP_SHAPES for k in KINDS if n < FORM_BIG_N or k == "gauss"}
# case id -> seed offset, as SEEDS above: with 70 queries ONE row within tau of a tie is 1.4 % (offsets 0, 1 and 2 have one such row, 3 has none)
FORM_SEEDS = {"70x300x1024-clustered": 3}
SLICE, MAX_SLICES, FUSED_MAX_D, CHUNK_ROWS = 512, 4096, 1024, 1024       # SSV_NN_LOOKUP_SLICE, _MAX_SLICES, _FUSED_MAX_D; the unfused route's query chunk


def lookup_plan(m, n, d, arith):
    """The launch plan of ssv_nn_lookup restated (csrc/nnlookup.hip: make_plan and the dispatch): {"fused", "bytes"} and, fused, T (query tiles), KT (tiles of a
    workgroup: the template argument), blocks, nch (64-column chunk trips), L (rows of a slice), P (slices); unfused, chunks (of queries) and parts (of the bank)."""
    cdiv, up = lambda a, b: -(-a // b), lambda v: (v + 255) // 256 * 256
    if arith == "bf16x3" and d % 32 == 0 and d <= FUSED_MAX_D:
        t, nch = cdiv(m, 32), cdiv(d, 64)
        kt = 1 if t == 1 else 2 if t == 2 else 4 if t <= 4 else 8
        rows = SLICE * cdiv(cdiv(n, SLICE), MAX_SLICES)
        p = cdiv(n, rows)
        return {"fused": True, "T": t, "KT": kt, "blocks": cdiv(t, kt), "nch": nch, "L": rows, "P": p, "bytes": 2 * up(p * 32 * t * 4) + 3 * 4 * nch * t * 1024}
    pc = cdiv(n, cdiv(n, min((1 << 26) // d, 65536)))
    cr = min(m, CHUNK_ROWS)
    return {"fused": False, "chunks": cdiv(m, cr), "parts": cdiv(n, pc), "bytes": 2 * up(m * 4) + up(cr * pc * 4)}


# (B, D, n): the loss cases
LOSS_SHAPES = ((8, 32, 16), (48, 96, 256), (130, 128, 1000))
TEMPERATURES = (0.1, 0.5)


def f32(v):
    """a scalar as the C ABI's float argument carries it"""
    return float(np.float32(float(v)))


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def lookup_inputs(name):
    """(queries [m, d], bank [n, d]) float32 numpy, rows of unit length.  gauss: Gaussian directions.  clustered: 50 unit centres, every row a centre plus 0.05
    Gaussian noise per coordinate, normalised - queries and bank rows of one cluster are near neighbours of each other."""
    if name in LOOKUP_CASES:
        c, seed = LOOKUP_CASES[name], 4000 + SEEDS.get(name, 0) + 31 * list(LOOKUP_CASES).index(name)
    else:
        c, seed = FORM_LOOKUP_CASES[name], 9000 + FORM_SEEDS.get(name, 0) + 31 * list(FORM_LOOKUP_CASES).index(name)
    g = torch.Generator().manual_seed(seed)
    if c.kind == "gauss":
        q, b = torch.randn(c.m, c.d, generator=g, dtype=torch.float64), torch.randn(c.n, c.d, generator=g, dtype=torch.float64)
    else:
        centres = _unit(torch.randn(50, c.d, generator=g, dtype=torch.float64))
        draw = lambda rows: centres[torch.randint(0, 50, (rows,), generator=g)] + 0.05 * torch.randn(rows, c.d, generator=g, dtype=torch.float64)
        q, b = draw(c.m), draw(c.n)
    return _unit(q).float().numpy(), _unit(b).float().numpy()


def scores(queries, bank):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(queries, np.float64) @ np.asarray(bank, np.float64).T


def tau(queries, bank):
    """[m] fp64: tau_i = 2^-14 |q_i| max_j |b_j|"""
    q, b = np.asarray(queries, np.float64), np.asarray(bank, np.float64)
    return EXCUSE * np.sqrt((q * q).sum(1)) * np.sqrt((b * b).sum(1)).max()


@functools.lru_cache(maxsize=None)
def lookup_reference(name):
    """{"s": S fp64 [m, n], "idx": first arg-max, "best", "margin": best minus second best (inf with one bank row), "tau", "excused": margin < tau}"""
    q, b = lookup_inputs(name)
    s = scores(q, b)
    idx = s.argmax(1)
    best = s[np.arange(s.shape[0]), idx]
    if s.shape[1] > 1:
        two = -np.partition(-s, 1, axis=1)[:, :2]
        margin = two[:, 0] - two[:, 1]
    else:
        margin = np.full(s.shape[0], np.inf)
    t = tau(q, b)
    return {"s": s, "idx": idx, "best": best, "margin": margin, "tau": t, "excused": margin < t}


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_inputs(b, d, n):
    """(z1, z2, p1, p2 [b, d], bank [n rounded up to 16, d]) float32 torch on the CPU.  The bank's first n rows are unit Gaussian directions, its pad rows zero (a
    MemoryBank); z2 and the predictions are noisy copies of z1, so the logits have a diagonal that stands out, as in training."""
    g = torch.Generator().manual_seed(7000 + b + 3 * d + 5 * n)
    z1 = torch.randn(b, d, generator=g)
    z2 = z1 + 0.5 * torch.randn(b, d, generator=g)
    p1 = 1.5 * z1 + 0.7 * torch.randn(b, d, generator=g)
    p2 = 0.5 * z2 + 0.7 * torch.randn(b, d, generator=g)
    bank = torch.zeros((n + 15) // 16 * 16, d)
    bank[:n] = _unit(torch.randn(n, d, generator=g, dtype=torch.float64)).float()
    return z1, z2, p1, p2, bank


def neighbours(bank, idx, temperature):
    """a = inv_T * bank[idx] in float32: one multiply per element, the lookup's nn output"""
    inv_t = torch.tensor(f32(1.0 / float(temperature)), dtype=torch.float32)
    return inv_t * bank[idx.long()]


def _pair(a, p):
    phat = p / p.norm(dim=1, keepdim=True).clamp_min(L2_EPS)
    logits = a @ phat.t()
    return (torch.logsumexp(logits, dim=1) - torch.diagonal(logits)).mean()


def loss_lines(p1, p2, a1, a2):
    return 0.5 * (_pair(a1, p2) + _pair(a2, p1))


def loss_reference(p1, p2, a1, a2, dtype):
    """{"loss" [1], "dp1", "dp2"} of the lines above in ``dtype`` on the CPU, the gradients by autograd; the inputs are the float32 values, widened"""
    p1, p2 = (t.detach().to(dtype).clone().requires_grad_(True) for t in (p1, p2))
    loss = loss_lines(p1, p2, a1.to(dtype), a2.to(dtype))
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dp1": p1.grad, "dp2": p2.grad}


def restated(p1, p2, a1, a2, dtype):
    """The same quantities from torch's own building blocks (F.normalize, F.cross_entropy): an independent restatement for the CPU self-check"""
    import torch.nn.functional as F
    p1, p2 = (t.detach().to(dtype).clone().requires_grad_(True) for t in (p1, p2))
    labels = torch.arange(p1.shape[0])
    loss = 0.5 * (F.cross_entropy(a1.to(dtype) @ F.normalize(p2, dim=1, eps=L2_EPS).t(), labels) + F.cross_entropy(a2.to(dtype) @ F.normalize(p1, dim=1, eps=L2_EPS).t(), labels))
    loss.backward()
    return {"loss": loss.detach().reshape(1), "dp1": p1.grad, "dp2": p2.grad}


def closed_form(p, a):
    """d l(a, p) / dp as the library forms it: dlogits = (softmax - I) / B, dP_hat = dlogits^T A, then the backward of the normalisation"""
    b = p.shape[0]
    norm = p.norm(dim=1, keepdim=True).clamp_min(L2_EPS)
    phat = p / norm
    dlog = (torch.softmax(a @ phat.t(), dim=1) - torch.eye(b, dtype=p.dtype)) / b
    dphat = dlog.t() @ a
    return (dphat - phat * (phat * dphat).sum(1, keepdim=True)) / norm


def errors(got, ref):
    """(e, m): relative L2 and max-norm error of got against ref (float64 tensors of one shape)"""
    got, ref = got.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    diff = got - ref
    return float(diff.norm() / ref.norm()), float(diff.abs().max() / ref.abs().max())
