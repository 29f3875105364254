"""fp64 CPU oracle of W-MSE (Ermolov et al., ICML 2021) for tests/test_wmse_cpu.py and tests/test_gpu_wmse.py: the block whitening through
torch.linalg.cholesky / solve_triangular under autograd (the backward is autograd's), the loss given a permutation, a Python restatement of the Philox keys
behind ssv_wmse_perm, and the fixed case generator.  ``dtype=torch.float32`` runs the same lines in fp32 (the reference the accuracy rule compares with)."""
import math

import numpy as np
import torch

# (blocks, w, d): the smallest shape, a width that is no multiple of 32, w barely above d, the CIFAR configuration, the widest
CASES = [(2, 8, 4), (5, 24, 12), (3, 40, 36), (4, 128, 64), (1, 136, 128), (2, 256, 128)]
# the launch forms (tests/test_gpu_whiten_forms.py): every (LDS tier, k-split) form of csrc/whiten.hip's lds_layout, both tier boundaries, row-class counts that are
# no power of two, and row counts that are no multiple of the 4 (forward) or 2 (backward) rows a thread owns
FORM_CASES = [(3, 9, 4), (2, 7, 4), (2, 29, 24), (2, 37, 28), (2, 45, 36), (2, 50, 44), (2, 53, 48), (2, 61, 52), (2, 67, 56), (2, 81, 68), (2, 99, 88), (1, 101, 88),
              (1, 103, 92), (1, 150, 124), (1, 1021, 128), (1, 1024, 128), (2, 1023, 8)]
SEEDS = (0, 1, 2)
EPSES = (0.0, 1e-3)
# (blocks, w, d) that ssv_whiten_workspace_bytes / _fwd / _bwd refuse: no block, d = 0 / below 4 / no multiple of 4 / above 128, w = d, w < d, w above 1024, blocks * w >= 2^31, negative
REFUSED_SHAPES = [(0, 128, 64), (8, 128, 0), (8, 128, 2), (8, 128, 66), (8, 256, 132), (8, 64, 64), (8, 32, 64), (8, 1025, 64), (1 << 22, 1024, 64), (-1, 128, 64)]
PERM_VIEW_BASE = 2048        # the Philox view key of iteration t is PERM_VIEW_BASE + t (the augmentation streams use 0 .. 1024 + views)


def lds_layout(d, bwd=False):
    """csrc/whiten.hip's lds_layout restated: {"kp" (k-split of the d x d products), "P" (row classes of the column means), "total" (bytes of LDS), "tier" (the
    instantiation that holds it)}.  The forward stages 32 rows of one operand, the backward 16 rows of two: the same bytes."""
    ld, tiles, threads = d + 1, (d // 4) ** 2, 1024
    kp = 1
    while kp < 16 and 2 * kp * tiles <= threads:
        kp *= 2
    p = min(16, threads // d)
    r16 = lambda v: (v + 15) // 16 * 16
    mat, chunk = r16(d * ld * 4), r16((16 if bwd else 32) * ld * 4)
    total = 2 * mat + (d * d * 8 if kp > 1 else 0) + chunk * (2 if bwd else 1) + d * 4 + d * 8 + p * d * 8 + d * 4
    return {"kp": kp, "P": p, "total": total, "tier": 16384 if total <= 16384 else 65536 if total <= 65536 else 163840}


def make_case(blocks, w, d, seed):
    """x [blocks * w][d] fp32 (drawn in fp64 from a seeded generator, then rounded): correlated columns of scale 0.5 .. 2 around means ten times the scale"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * blocks + 3 * w + d)
    n = blocks * w
    z = torch.randn(n, d, generator=g, dtype=torch.float64)
    mix = torch.eye(d, dtype=torch.float64) + 0.3 * torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d)
    scale = torch.linspace(0.5, 2.0, d, dtype=torch.float64)
    signs = torch.randint(0, 2, (d,), generator=g).to(torch.float64) * 2.0 - 1.0
    return ((z @ mix) * scale + 10.0 * scale * signs).to(torch.float32)


def make_rows(blocks, w, seed):
    """int32 [blocks][w]: a seeded permutation of 0 .. blocks * w - 1, cut into blocks"""
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randperm(blocks * w, generator=g).to(torch.int32).view(blocks, w)


def whiten_block(xb, eps):
    """(y, mean, W) of one block xb [w][d] in xb's dtype; differentiable"""
    w, d = xb.shape
    mu = xb.mean(dim=0)
    xc = xb - mu
    s = xc.T @ xc / (w - 1)
    a = (1.0 - eps) * s + eps * torch.eye(d, dtype=xb.dtype)
    l = torch.linalg.cholesky(a)
    winv = torch.linalg.solve_triangular(l, torch.eye(d, dtype=xb.dtype), upper=False)
    return xc @ winv.T, mu, winv


def whiten(x, rows, eps, dtype=torch.float64):
    """(y [blocks * w][d], mean [blocks][d], winv [blocks][d][d]) of x [n_rows][d] by the blocks rows [blocks][w]; y is differentiable in the returned ``xin``"""
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    ys, mus, ws = [], [], []
    for b in range(rows.shape[0]):
        y, mu, wi = whiten_block(xin[rows[b].long()], eps)
        ys.append(y), mus.append(mu), ws.append(wi)
    return torch.cat(ys), torch.stack(mus), torch.stack(ws), xin


def whiten_with_grad(x, rows, eps, dy, dtype=torch.float64):
    """{y, mean, winv, dx} with dx = d <dy, y> / dx by autograd ([n_rows][d]; rows no block names stay 0)"""
    y, mu, wi, xin = whiten(x, rows, eps, dtype)
    (dx,) = torch.autograd.grad((y * dy.to(dtype)).sum(), xin)
    return {"y": y.detach(), "mean": mu.detach(), "winv": wi.detach(), "dx": dx}


def cov_err(y, blocks, w):
    """|y^T y / (w - 1) - I| [blocks][d][d] of a block-dense y, in fp64"""
    yb = y.to(torch.float64).view(blocks, w, -1)
    return (yb.transpose(1, 2) @ yb / (w - 1) - torch.eye(yb.shape[2], dtype=torch.float64)).abs()


def closed_form_bwd(xb, eps, g):
    """dx of one block by the closed form of include/ssv_hip.h (ssv_whiten_bwd), in xb's dtype: an independent restatement of autograd's backward"""
    w, d = xb.shape
    y, mu, wi = whiten_block(xb, eps)
    xc = xb - mu
    l = torch.linalg.inv(wi)
    dw = g.T @ xc
    dl = torch.tril(-wi.T @ dw @ wi.T)
    p = torch.tril(l.T @ dl)
    p = p - 0.5 * torch.diag(torch.diagonal(p))
    da = wi.T @ p @ wi
    da = 0.5 * (da + da.T)
    gg = g @ wi + 2.0 * (1.0 - eps) / (w - 1) * xc @ da
    return gg - gg.mean(dim=0)


def whiten_eigh(xb, eps):
    """ZCA whitening through eigh: another whitening of the same covariance, so y^T y agrees with the Cholesky whitening's"""
    w, d = xb.shape
    xc = xb - xb.mean(dim=0)
    a = (1.0 - eps) * (xc.T @ xc / (w - 1)) + eps * torch.eye(d, dtype=xb.dtype)
    lam, v = torch.linalg.eigh(a)
    return xc @ (v / lam.sqrt()) @ v.T


def wmse_loss(z1, z2, perm, w_size, eps, dtype=torch.float64, whitener=None):
    """(loss, dz1, dz2): perm int [iters][2][N]; per iteration the first nb * w_size entries of perm[t][0] and perm[t][1] (indices into cat(z1, z2)) cut into runs of
    w_size, each whitened alone; term = 2 - 2 mean_p cos(y1_p, y2_p); the mean over iterations"""
    a = z1.detach().to(dtype).clone().requires_grad_(True)
    b = z2.detach().to(dtype).clone().requires_grad_(True)
    h = torch.cat([a, b])
    n = z1.shape[0]
    nb = n // w_size
    wh = whitener or (lambda t: whiten_block(t, eps)[0])
    total = 0.0
    for t in range(perm.shape[0]):
        ys = []
        for v in range(2):
            idx = perm[t][v][:nb * w_size].long().view(nb, w_size)
            ys.append(torch.cat([wh(h[idx[k]]) for k in range(nb)]))
        c = torch.nn.functional.cosine_similarity(ys[0], ys[1], dim=1, eps=0.0)
        total = total + (2.0 - 2.0 * c.mean())
    loss = total / perm.shape[0]
    da, db = torch.autograd.grad(loss, (a, b))
    return loss.detach(), da, db


# ---- the Philox4x32-10 keys of ssv_wmse_perm (csrc/philox.h: key = seed, counter = (position, view key << 16, step, 0); the first word of the block)
def philox_first_word(seed, step, sample, view):
    m = 0xFFFFFFFF
    k0, k1 = seed & m, (seed >> 32) & m
    x0, x1, x2, x3 = sample & m, ((sample >> 32) & 0xFFFF) | ((view & 0xFFFF) << 16), step & m, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        x0, x1, x2, x3 = ((p1 >> 32) ^ x1 ^ k0) & m, p1 & m, ((p0 >> 32) ^ x3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return x0


def perm_keys(n, seed, step, t):
    return np.array([philox_first_word(seed, step, i, PERM_VIEW_BASE + t) for i in range(n)], dtype=np.uint64)


def perm(n, views, iters, seed, step):
    """int32 [iters][views][n]: positions sorted by their key, ties to the lower position; view v adds v * n"""
    out = np.empty((iters, views, n), dtype=np.int32)
    for t in range(iters):
        order = np.argsort(perm_keys(n, seed, step, t), kind="stable").astype(np.int32)
        for v in range(views):
            out[t, v] = order + v * n
    return torch.from_numpy(out)


# ---- the accuracy rule's two figures (tests/test_gpu_loss_kernels.py, rule (a)): e = ||x - ref64||_2 / ||ref64||_2 and m = max|x - ref64| / max|ref64|
def errs(got, ref64):
    ref64 = ref64.detach().to(torch.float64).cpu()
    diff = got.detach().to(torch.float64).cpu() - ref64
    return float(diff.norm() / ref64.norm().clamp_min(1e-300)), float(diff.abs().max() / ref64.abs().max().clamp_min(1e-300))
