"""Loss modules of the accelerated path with the reference's constructor signatures
(utils/losses.py:8-46 SimclrLoss, :120-142 BarlowLoss; BYOL uses nn.MSELoss, models/byol.py:89).  VicregLoss has no counterpart there.

Each forward runs the fused HIP kernels (forward AND the gradient w.r.t. the embeddings), and
returns a 0-d tensor wired into torch.autograd so ``loss.backward()`` hands dz to the heads.
With a process group, the embeddings are all-gathered over RCCL so NT-Xent sees global negatives.
"""
import torch
import torch.nn as nn

from .. import _lib, ops
from .. import distributed as hdist


def _pad32(d):
    return (d + 31) // 32 * 32


class _NTXentFn(torch.autograd.Function):
    """NT-Xent over the GLOBAL batch.  Each rank normalises its rows straight into their slots of the gathered
    matrix Z = [zi_all ; zj_all], all-gathers the slots (RCCL), computes the log-sum-exp of ITS rows against all
    columns, and - because S is symmetric - needs only the all-gathered row LSEs to form the exact gradient of the
    global-mean loss w.r.t. its own rows (option iii): TWO small collectives per step - one all-gather of [zi ; zj], one of
    the row LSEs with the loss partial riding along - and no redundant Gram work."""

    @staticmethod
    def forward(ctx, zi, zj, normalize, temperature):
        b, d = zi.shape
        ld = _pad32(d)
        wide = ld > 128                  # beyond the register-resident kernels: Gram block through the GEMM kernels (any width)
        world, rank = hdist.world_size(), hdist.rank()
        nglob, seg0 = b * world, b * rank
        rows = (2 * nglob + 15) // 16 * 16 if wide else 2 * nglob          # wide: the row count is a GEMM dimension (multiple of 16)
        zall = torch.empty((rows, ld), dtype=torch.float32, device=zi.device)
        if rows > 2 * nglob:
            ops.fill_(zall[2 * nglob:], 0.0)
        exchange = hdist.is_on()          # also with a forced world of one rank (the single-GPU functional test of the RCCL calls)
        if exchange:
            # ONE all-gather for both views: every rank normalises into its [zi_r ; zj_r] block, the blocks are gathered in rank order and
            # re-laid as [zi_all ; zj_all] (the layout the row kernels index: row r < N pairs with row r + N)
            loc = torch.empty((2 * b, ld), dtype=torch.float32, device=zi.device)
            _, inv_i = ops.l2norm_fwd(zi.detach().contiguous(), normalize, ld, out=loc[:b])
            _, inv_j = ops.l2norm_fwd(zj.detach().contiguous(), normalize, ld, out=loc[b:])
            blocks = torch.empty((world * 2 * b, ld), dtype=torch.float32, device=zi.device)
            hdist.all_gather_blocks(blocks, loc)
            zall[:2 * nglob].view(2, world, b, ld).copy_(blocks.view(world, 2, b, ld).permute(1, 0, 2, 3))
        else:
            _, inv_i = ops.l2norm_fwd(zi.detach().contiguous(), normalize, ld, out=zall[seg0:seg0 + b])
            _, inv_j = ops.l2norm_fwd(zj.detach().contiguous(), normalize, ld, out=zall[nglob + seg0:nglob + seg0 + b])
        inv_t = 1.0 / float(temperature)
        gram = None
        if wide:
            zloc = torch.cat((zall[seg0:seg0 + b], zall[nglob + seg0:nglob + seg0 + b]), 0)
            gram = ops.conv2d_fwd(zloc.view(2 * b, 1, 1, ld), zall).view(2 * b, rows)          # S = Z_loc Z_all^T on the MFMA GEMM
            lse_loc, pos_loc = ops.ntxent_gram_fwd(gram, nglob, b, seg0, inv_t)
        else:
            lse_loc, pos_loc = ops.ntxent_fwd(zall, nglob, b, seg0, inv_t)
        loss = ops.ntxent_loss(lse_loc, pos_loc, 1.0 / (2 * nglob))
        if exchange:
            # ONE all-gather for the row log-sum-exps of both views; this rank's share of the loss rides along as one more float, so every
            # rank sums the same `world` partials in the same order (the global-batch loss, identical on all ranks, no all-reduce)
            pack = torch.empty((1, 2 * b + 4), dtype=torch.float32, device=zi.device)
            pack[0, :2 * b].copy_(lse_loc)
            pack[0, 2 * b:].copy_(loss.expand(4))
            got = torch.empty((world, 2 * b + 4), dtype=torch.float32, device=zi.device)
            hdist.all_gather_blocks(got, pack)
            loss = got[:, 2 * b].sum()
            lse_all = torch.empty((2 * nglob,), dtype=torch.float32, device=zi.device)
            lse_all.view(2, world, b).copy_(got[:, :2 * b].view(world, 2, b).permute(1, 0, 2))
        else:
            lse_all = lse_loc
        ctx.saved = (zall, lse_all, inv_i, inv_j, nglob, b, seg0, d, inv_t, bool(normalize), gram)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        zall, lse_all, inv_i, inv_j, nglob, b, seg0, d, inv_t, normalize, gram = ctx.saved
        if gram is not None:             # wide embeddings: W' in place over the Gram block, then dZ = W' Z_all as a GEMM
            ops.ntxent_gram_weights(gram, lse_all, nglob, b, seg0, inv_t, inv_t / (2 * nglob))
            dzall = ops.conv2d_dgrad(gram.view(2 * b, 1, 1, -1), zall, (2 * b, 1, 1, zall.shape[1])).view(2 * b, zall.shape[1])
        else:
            dzall = ops.ntxent_bwd(zall, lse_all, nglob, b, seg0, inv_t, inv_t / (2 * nglob))
        ops.scale_(dzall, dloss.contiguous())                # chain rule with the upstream scalar, read on the device
        dzi = ops.l2norm_bwd(zall[seg0:seg0 + b], inv_i, dzall[:b], d, normalize)
        dzj = ops.l2norm_bwd(zall[nglob + seg0:nglob + seg0 + b], inv_j, dzall[b:], d, normalize)
        return dzi, dzj, None, None


class SimclrLoss(nn.Module):
    """NT-Xent (utils/losses.py:8-46): defaults normalize=False, temperature=1.0 like the reference."""

    def __init__(self, normalize=False, temperature=1.0):
        super().__init__()
        self.normalize = normalize
        self.temperature = temperature

    def forward(self, zi, zj):
        if zi.shape != zj.shape or zi.dim() != 2:
            raise ValueError(f"SimclrLoss expects two [N,D] matrices, got {tuple(zi.shape)} and {tuple(zj.shape)}")
        return _NTXentFn.apply(zi, zj, self.normalize, self.temperature)


class _MSEPairFn(torch.autograd.Function):
    """Data parallel: the mean runs over the GLOBAL batch (scale 1/(B_local*world*D)) and the scalar is all-reduced, so the
    SUM of per-rank parameter gradients is the large-batch gradient - the same convention as the other two losses."""

    @staticmethod
    def forward(ctx, o1, o2, t1, t2):
        o1c, o2c, t1c, t2c = (t.detach().contiguous() for t in (o1, o2, t1, t2))
        loss, do1, do2 = ops.mse_pair(o1c, o2c, t1c, t2c, 1.0 / (o1c.numel() * hdist.world_size()))
        hdist.all_reduce_sum(loss)
        ctx.saved = (do1, do2)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        do1, do2 = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(do1, g), ops.scale_(do2, g), None, None


def byol_pair_loss(online_1, online_2, target_1, target_2):
    """MSE(online_1, target_2) + MSE(online_2, target_1), each a mean over B*D (models/byol.py:129-130)."""
    return _MSEPairFn.apply(online_1, online_2, target_1, target_2)


class _BarlowFn(torch.autograd.Function):
    """Whole Barlow Twins loss + its gradient w.r.t. both embedding matrices, composed from the C ABI:
    [F.normalize] -> column standardisation (BN kernels, gamma = sqrt((B-1)/B), eps = 0 = unbiased std without eps)
    -> Craw = zi_hat^T zj_hat (wgrad-shaped MFMA GEMM over the batch) -> loss / G (ssv_barlow_cgrad)
    -> d zi_hat = zj_hat G^T (fwd-shaped GEMM), d zj_hat = zi_hat G (dgrad-shaped GEMM) -> BN backward [-> normalize backward].
    Data parallel: the embeddings are all-gathered and every rank evaluates the global-batch loss redundantly
    (3 GEMMs of B x D x D - cheaper than a 64 MB all-reduce of C), then keeps the gradient rows of its own samples."""

    @staticmethod
    def forward(ctx, zi, zj, normalize, lmbda):
        bl, d = zi.shape
        if d % 16:
            raise _lib.SsvError(f"BarlowLoss: projection dim must be a multiple of 16 (got {d})")
        world, rank = hdist.world_size(), hdist.rank()
        b = bl * world
        dev = zi.device
        zs = []
        for z in (zi, zj):
            zall = torch.empty((b, d), dtype=torch.float32, device=dev)
            zall[rank * bl:(rank + 1) * bl].copy_(z.detach())
            if world > 1:
                hdist.all_gather_rows(zall, bl)
            zs.append(zall)
        invs = [None, None]
        if normalize:
            for k in range(2):
                zs[k], invs[k] = ops.l2norm_fwd(zs[k], True)
        gamma = ops.fill_(torch.empty(d, dtype=torch.float32, device=dev), ((b - 1) / b) ** 0.5)
        beta = ops.fill_(torch.empty(d, dtype=torch.float32, device=dev), 0.0)
        hats, stats = [], []
        for k in range(2):
            y, mean, invstd = ops.bn_train_fwd(zs[k], gamma, beta, None, None, None, relu=False, eps=0.0)
            hats.append(y)
            stats.append((mean, invstd))
        craw = torch.empty((d, d), dtype=torch.float32, device=dev)
        ops.conv2d_wgrad(hats[1].view(b, 1, 1, d), hats[0].view(b, 1, 1, d), craw, craw, accumulate=False)   # craw[i][j] = sum_b zi_hat[b,i] zj_hat[b,j]
        loss, g = ops.barlow_cgrad(craw, 1.0 / b, lmbda)
        dhat_i = ops.conv2d_fwd(hats[1].view(b, 1, 1, d), g).view(b, d)                     # [b,i] = sum_j zj_hat[b,j] G[i,j]
        dhat_j = ops.conv2d_dgrad(hats[0].view(b, 1, 1, d), g, (b, 1, 1, d)).view(b, d)     # [b,j] = sum_i zi_hat[b,i] G[i,j]
        dgam, dbet = torch.empty(d, dtype=torch.float32, device=dev), torch.empty(d, dtype=torch.float32, device=dev)
        grads = []
        for k, dh in enumerate((dhat_i, dhat_j)):
            dz, _ = ops.bn_train_bwd(dh, None, zs[k], gamma, stats[k][0], stats[k][1], False, dgam, dbet, accumulate=False)
            if normalize:
                dz = ops.l2norm_bwd(zs[k], invs[k], dz, d, True)
            grads.append(dz[rank * bl:(rank + 1) * bl])
        ctx.saved = grads
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dzi, dzj = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(dzi.contiguous(), g), ops.scale_(dzj.contiguous(), g), None, None


class BarlowLoss(nn.Module):
    """Barlow Twins loss (utils/losses.py:120-142): defaults normalize=True, off_diagonal_weight=0.005 like the reference."""

    def __init__(self, normalize=True, off_diagonal_weight=0.005):
        super().__init__()
        self.normalize = normalize
        self.lmbda = off_diagonal_weight

    def forward(self, z_i, z_j):
        if z_i.shape != z_j.shape or z_i.dim() != 2:
            raise ValueError(f"BarlowLoss expects two [B,D] matrices, got {tuple(z_i.shape)} and {tuple(z_j.shape)}")
        return _BarlowFn.apply(z_i, z_j, self.normalize, self.lmbda)


class _VicregFn(torch.autograd.Function):
    """Whole VICReg loss + its gradient w.r.t. both embedding matrices, composed from the C ABI (csrc/vicreg.hip states the formulas):
    ssv_vicreg_prep (centred views, std, the element-wise gradient part e, the sim and std terms) -> Craw[v] = xc[v]^T xc[v] (wgrad-shaped MFMA GEMM over
    the batch) -> ssv_vicreg_cgrad (cov term, the loss, G in place over Craw) -> d[v] = xc[v] G[v] + e[v] (fwd-shaped GEMM, e as its epilogue addend; G is
    symmetric).  The centring has no backward of its own: both terms in xc have zero column mean."""

    @staticmethod
    def forward(ctx, x, y, module):
        b, d = x.shape
        xc, _, e, parts = ops.vicreg_prep(x.detach().contiguous(), y.detach().contiguous(), module.sim_coeff, module.std_coeff, module.cov_coeff, module.eps)
        craw = torch.empty((2, d, d), dtype=torch.float32, device=x.device)
        for v in range(2):
            ops.conv2d_wgrad(xc[v].view(b, 1, 1, d), xc[v].view(b, 1, 1, d), craw[v], craw[v], accumulate=False)      # craw[v][i][j] = sum_b xc[v][b,i] xc[v][b,j]
        loss, g = ops.vicreg_cgrad(craw, b, module.cov_coeff, parts)
        ctx.saved = tuple(ops.conv2d_fwd(xc[v].view(b, 1, 1, d), g[v], addend=e[v].view(b, 1, 1, d)).view(b, d) for v in range(2))
        ops.drop_planes(g)                   # G is no weight: its bf16 planes (and craw's storage with them) must not wait in the cache for the next optimizer step
        module.terms = loss[1:4]
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        dx, dy = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(dx, g), ops.scale_(dy, g), None


class VicregLoss(nn.Module):
    """VICReg (Bardes, Ponce, LeCun 2022; not in the reference): sim_coeff * invariance + std_coeff * variance hinge + cov_coeff * off-diagonal covariance
    of two [B, D] embedding matrices, D a multiple of 32 and B >= 2.  ``terms`` holds the three weighted terms of the last forward as a device tensor."""

    def __init__(self, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4):
        super().__init__()
        self.sim_coeff, self.std_coeff, self.cov_coeff, self.eps = float(sim_coeff), float(std_coeff), float(cov_coeff), float(eps)
        self.terms = None

    def forward(self, x, y):
        if x.dim() != 2 or y.dim() != 2 or x.shape != y.shape:
            raise ValueError(f"VicregLoss expects two [B,D] matrices, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.shape[0] < 2 or x.shape[1] % 32 or x.shape[1] > _lib.VICREG_MAX_D:
            raise ValueError(f"VicregLoss needs B >= 2 and D a multiple of 32 up to {_lib.VICREG_MAX_D}, got {tuple(x.shape)}")
        if hdist.is_on() and hdist.world_size() > 1:
            raise NotImplementedError("VicregLoss is single-process: the batch statistics are not gathered across ranks")
        return _VicregFn.apply(x, y, self)


def nnclr_pair(a, p, labels):
    """One direction of the NNCLR loss and its gradient: (stats, dp) with stats[0] = mean_i CE_i(A P_hat^T) - ``a`` [B, D] the neighbours already scaled by 1 / T,
    P_hat = l2norm(p) - and dp = d stats[0] / dp.  Row-direction cross-entropy only (the paper's eq. 3)."""
    b, d = p.shape
    bp = (b + 3) // 4 * 4                    # the weight-gradient GEMM takes whole float4s of dlogits: the logit matrix is [B, bp], its pad columns products with zero rows
    phat = torch.empty((bp, d), dtype=torch.float32, device=p.device)
    if bp > b:
        ops.fill_(phat[b:], 0.0)
    _, inv = ops.l2norm_fwd(p, True, out=phat[:b])
    a4 = a.view(b, 1, 1, d)
    logits = ops.conv2d_fwd(a4, phat).view(b, bp)                                     # logits[i][j] = a_i . p_hat_j
    stats, dlog = ops.softmax_ce(logits, labels, classes=b)                           # the pad columns of dlogits are zeros
    dphat = torch.empty_like(phat)
    ops.conv2d_wgrad(a4, dlog.view(b, 1, 1, bp), phat, dphat, accumulate=False)         # dP_hat = dlogits^T A
    dp = ops.l2norm_bwd(phat[:b], inv, dphat[:b], d, True)
    ops.drop_planes(phat)                    # P_hat is no weight: its bf16 planes must not wait in the cache for the next optimizer step
    return stats, dp


class _NnclrFn(torch.autograd.Function):
    """Lookup (both views' embeddings, stacked: the bank is read once per step), the two cross-entropies and their gradients in forward; backward only scales."""

    @staticmethod
    def forward(ctx, p1, p2, z1, z2, bank, queue_size, module):
        b, d = p1.shape
        zq = torch.empty((2 * b, d), dtype=torch.float32, device=p1.device)
        ops.l2norm_fwd(z1.detach().contiguous(), True, out=zq[:b])
        ops.l2norm_fwd(z2.detach().contiguous(), True, out=zq[b:])
        nn_, module.last_idx, module.last_sim = ops.nn_lookup(zq, bank, n=queue_size, out_scale=1.0 / module.temperature)
        labels = torch.arange(b, dtype=torch.int32, device=p1.device)
        s12, dp2 = nnclr_pair(nn_[:b], p2.detach().contiguous(), labels)               # (nn1, p2)
        s21, dp1 = nnclr_pair(nn_[b:], p1.detach().contiguous(), labels)               # (nn2, p1)
        half = torch.full((1,), 0.5, dtype=torch.float32, device=p1.device)
        loss = ops.scale_(ops.add_(s12[:1], s21[:1]), half)
        ctx.saved = (ops.scale_(dp1, half), ops.scale_(dp2, half))
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        dp1, dp2 = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(dp1, g), ops.scale_(dp2, g), None, None, None, None, None


class NnclrLoss(nn.Module):
    """NNCLR (Dwibedi et al., ICCV 2021; not in the reference): 1/2 (CE(NN(z1) . p2^T / T) + CE(NN(z2) . p1^T / T)) with NN(z) the nearest neighbour of the
    normalised, detached projection in the support queue ``bank`` [>= queue_size, D] (models.moco.MemoryBank) and p the L2-normalised predictions.  Gradients reach
    p1 and p2 only.  D % 4 == 0 (a multiple of 32 takes the fused lookup).  ``last_idx`` (device int32 [2B]) / ``last_sim``: the neighbours of the last forward."""

    def __init__(self, temperature=0.1):
        super().__init__()
        self.temperature = float(temperature)
        if not self.temperature > 0.0:
            raise ValueError(f"NnclrLoss: the temperature must be positive (got {temperature})")
        self.last_idx = self.last_sim = None

    def forward(self, z1, z2, p1, p2, bank, queue_size=None):
        shapes = {tuple(t.shape) for t in (z1, z2, p1, p2)}
        if p1.dim() != 2 or len(shapes) != 1:
            raise ValueError(f"NnclrLoss expects four [B,D] matrices of one shape, got {[tuple(t.shape) for t in (z1, z2, p1, p2)]}")
        n = bank.shape[0] if queue_size is None else int(queue_size)
        if bank.dim() != 2 or bank.shape[1] != p1.shape[1] or not 1 <= n <= bank.shape[0] or p1.shape[1] % 4 or 2 * p1.shape[0] > _lib.NN_LOOKUP_MAX_M:
            raise ValueError(f"NnclrLoss needs a bank [>= queue_size, D] with D % 4 == 0 and B <= {_lib.NN_LOOKUP_MAX_M // 2}, got bank {tuple(bank.shape)}, "
                             f"queue_size {n}, embeddings {tuple(p1.shape)}")
        if hdist.is_on():
            raise NotImplementedError("NnclrLoss is single-process: the support queue is not replicated across ranks")
        return _NnclrFn.apply(p1, p2, z1, z2, bank, n, self)


class _WmseTermFn(torch.autograd.Function):
    """One iteration of W-MSE: the blocks of both views whitened in ONE call, the pairs normalised and compared, and the whole backward down to dh in forward;
    backward only scales.  Rows of h that no block names (a ragged batch) get zero gradient."""

    @staticmethod
    def forward(ctx, h, rows, eps, module):
        hc = h.detach().contiguous()
        y, mean, winv, info = ops.whiten_fwd(hc, rows, eps)
        module.last_info.append(info)
        m, d = y.shape[0] // 2, y.shape[1]
        y1, y2 = y[:m], y[m:]
        n1, inv1 = ops.l2norm_fwd(y1, True)
        n2, inv2 = ops.l2norm_fwd(y2, True)
        # |n1 - n2|^2 = 2 - 2 cos per pair: ops.mse_pair returns scale * 2 sum_p |n1_p - n2_p|^2 and, as do1 / do2, the gradients of scale * sum_p |n1_p - n2_p|^2
        # through ONE of the two (symmetric) terms each - so with scale = 1 / m the gradients are those of the mean and the loss is twice it
        loss2, dn1, dn2 = ops.mse_pair(n1, n2, n1, n2, 1.0 / m)
        half = torch.full((1,), 0.5, dtype=torch.float32, device=h.device)
        loss = ops.scale_(loss2.view(1), half)
        dy = torch.cat([ops.l2norm_bwd(n1, inv1, dn1, d, True), ops.l2norm_bwd(n2, inv2, dn2, d, True)])
        ctx.saved = ops.whiten_bwd(hc, rows, eps, mean, winv, dy)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        return ops.scale_(ctx.saved, dloss.contiguous()), None, None, None


class WmseLoss(nn.Module):
    """W-MSE (Ermolov et al., ICML 2021; not in the reference), called as fn(z1, z2) with the [N, d] projections of the two views.  h = cat(z1, z2); per iteration t
    (``w_iter`` of them) a device permutation of the batch (ops.wmse_perm, keyed by (seed, step, t); the step counter is a device tensor owned by this module and
    advanced by every call, so a replayed step draws a new permutation) cuts each view into nb = N // w_size blocks of ``w_size`` rows - the same rows in both views, so
    position p of the view-1 half is the positive of position p of the view-2 half - each block is whitened alone (ops.whiten_fwd, ``eps`` shrinks the covariance towards
    I) and the term is 2 - 2 mean_p cos(y1_p, y2_p).  The loss is the mean of the terms.  A ragged batch trains on nb * w_size of its rows per iteration.
    ``check=True`` (the eager default) reads the whitening's status back - one host synchronisation - and raises SsvError naming the block whose covariance has no
    Cholesky factor; a step graph passes False.  ``last_perm``: the permutation tensor of the last call; ``last_info``: the status tensors of its iterations."""

    def __init__(self, w_size, w_iter=1, eps=0.0, seed=0):
        super().__init__()
        self.w_size, self.w_iter, self.eps, self.seed = int(w_size), int(w_iter), float(eps), int(seed)
        if not 1 <= self.w_iter <= _lib.WMSE_PERM_MAX_ITERS:
            raise ValueError(f"WmseLoss: w_iter must be in [1, {_lib.WMSE_PERM_MAX_ITERS}] (got {w_iter})")
        if not 0.0 <= self.eps < 1.0:
            raise ValueError(f"WmseLoss: eps must be in [0, 1) (got {eps})")
        if not 2 <= self.w_size <= _lib.WHITEN_MAX_W:
            raise ValueError(f"WmseLoss: w_size must be in [2, {_lib.WHITEN_MAX_W}] (got {w_size})")
        self.step_dev = None
        self.last_perm, self.last_info = None, []

    def reset_step(self, device, step=0):
        """(re)create the device step counter: a trainer calls this once, before any step is captured into a graph"""
        self.step_dev = torch.full((1,), int(step), dtype=torch.int64, device=device)
        return self

    def forward(self, z1, z2, check=True):
        if z1.dim() != 2 or z1.shape != z2.shape:
            raise ValueError(f"WmseLoss expects two [N,d] matrices of one shape, got {tuple(z1.shape)} and {tuple(z2.shape)}")
        n, d = z1.shape
        if d < 4 or d % 4 or d > _lib.WHITEN_MAX_D:
            raise ValueError(f"WmseLoss: the embedding width must be a multiple of 4 in [4, {_lib.WHITEN_MAX_D}] (got {d})")
        if self.w_size <= d:
            raise ValueError(f"WmseLoss: w_size ({self.w_size}) must exceed the embedding width ({d}): the covariance of a block would be singular")
        if n < self.w_size or n > _lib.WMSE_PERM_MAX_N:
            raise ValueError(f"WmseLoss: the batch ({n}) must hold at least one block of w_size = {self.w_size} rows and at most {_lib.WMSE_PERM_MAX_N} rows")
        if hdist.is_on():
            raise NotImplementedError("WmseLoss is single-process: the sub-batches are drawn from one rank's batch")
        if self.step_dev is None or self.step_dev.device != z1.device:
            self.reset_step(z1.device)
        nb = n // self.w_size
        self.last_perm = perm = ops.wmse_perm(n, 2, self.w_iter, self.seed, step_dev=self.step_dev)
        self.last_info = []
        h = torch.cat([z1, z2])
        total = None
        for t in range(self.w_iter):
            rows = perm[t, :, :nb * self.w_size].reshape(2 * nb, self.w_size).contiguous()
            term = _WmseTermFn.apply(h, rows, self.eps, self)
            total = term if total is None else total + term
        if check:
            for t, info in enumerate(self.last_info):
                bad = info.cpu()
                if int((bad != 0).sum()):
                    b = int((bad != 0).nonzero()[0])
                    raise _lib.SsvError(f"WmseLoss: iteration {t}, block {b} (view {b // nb + 1}, sub-batch {b % nb}): whitening status {int(bad[b])} "
                                        "(j + 1: pivot j of the covariance's Cholesky factor is not positive; -1: an index out of range)")
        return total if self.w_iter == 1 else total / self.w_iter


# ------------------------------------------------------------------------------------------- sibling algorithms
class _NegDotPairFn(torch.autograd.Function):
    """0.5 * (SimSiamLoss(o1, t2) + SimSiamLoss(o2, t1)) (utils/losses.py:145-152, models/simsiam.py:126-127); the mean runs over
    the GLOBAL batch under data parallelism (weight 1/world, scalar all-reduced)."""

    @staticmethod
    def forward(ctx, o1, o2, t1, t2):
        o1c, o2c, t1c, t2c = (t.detach().contiguous() for t in (o1, o2, t1, t2))
        loss, do1, do2 = ops.negdot_pair(o1c, o2c, t1c, t2c, 0.5 / (o1c.shape[0] * hdist.world_size()))
        hdist.all_reduce_sum(loss)
        ctx.saved = (do1, do2)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        do1, do2 = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(do1, g), ops.scale_(do2, g), None, None


def simsiam_pair_loss(online_1, online_2, target_1, target_2):
    return _NegDotPairFn.apply(online_1, online_2, target_1, target_2)


class _RelicKLFn(torch.autograd.Function):
    """alpha * KL term of RelicLoss (utils/losses.py:195-201) with its gradient w.r.t. all three embedding matrices."""

    @staticmethod
    def forward(ctx, zi, zj, zo, normalize, temperature, alpha):
        # Data parallel: the term soft-maxes the N diagonal logits ACROSS the batch, so the (normalised) embeddings are all-gathered and
        # every rank evaluates the global-batch term (N x D work - nothing next to the encoder), keeping the gradient rows of its own
        # samples: the SUM of the per-rank parameter gradients is the gradient of the global loss, like the other losses here.
        bl, d = zi.shape
        world, rank = hdist.world_size(), hdist.rank()
        mats, invs = [], []
        for z in (zi, zj, zo):
            zh, inv = ops.l2norm_fwd(z.detach().contiguous(), normalize)
            if world > 1:
                zall = torch.empty((bl * world, d), dtype=torch.float32, device=z.device)
                zall[rank * bl:(rank + 1) * bl].copy_(zh)
                zh = hdist.all_gather_rows(zall, bl)
            mats.append(zh)
            invs.append(inv)
        loss, *grads = ops.relic_kl(mats[0], mats[1], mats[2], 1.0 / float(temperature), alpha)
        mine = slice(rank * bl, (rank + 1) * bl)
        ctx.saved = tuple(ops.l2norm_bwd(mats[k][mine].contiguous(), invs[k], grads[k][mine].contiguous(), d, normalize) for k in range(3))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        g = dloss.contiguous()
        dzi, dzj, dzo = (ops.scale_(t, g) for t in ctx.saved)
        return dzi, dzj, dzo, None, None, None


class RelicLoss(nn.Module):
    """utils/losses.py:155-201: the NT-Xent of (zi, zj) plus alpha * the invariance term against the un-augmented image's embedding."""

    def __init__(self, normalize=True, temperature=1.0, alpha=0.5):
        super().__init__()
        self.normalize, self.temperature, self.alpha = normalize, temperature, alpha
        self.contrastive = SimclrLoss(normalize, temperature)

    def forward(self, zi, zj, z_orig):
        return self.contrastive(zi, zj) + _RelicKLFn.apply(zi, zj, z_orig, self.normalize, self.temperature, self.alpha)


class _MocoFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, keys, bank, queue_size, normalize, temperature):
        # Data parallel: every query is scored against its own key and the (replicated) queue - a per-sample loss, so the mean over the
        # GLOBAL batch is the local mean weighted 1/world with the scalar all-reduced (the convention of the BYOL pair loss); the queue
        # stays identical on every rank because MemoryBank.add_batch pushes the all-gathered keys in rank order.
        n, d = query.shape
        world = hdist.world_size()
        qn, inv_q = ops.l2norm_fwd(query.detach().contiguous(), normalize)
        kn, _ = ops.l2norm_fwd(keys.detach().contiguous(), normalize)
        neg = ops.conv2d_fwd(qn.view(n, 1, 1, d), bank).view(n, bank.shape[0])                    # [N, K_pad] products with the queue (MFMA GEMM)
        loss, dq = ops.moco_loss(qn, kn, neg, queue_size, 1.0 / float(temperature))
        ops.conv2d_dgrad(neg.view(n, 1, 1, -1), bank, (n, 1, 1, d), addend=dq.view(n, 1, 1, d), out=dq.view(n, 1, 1, d))   # dq += P . bank
        dz = ops.l2norm_bwd(qn, inv_q, dq, d, normalize)
        if world > 1:
            w = torch.full((), 1.0 / world, dtype=torch.float32, device=query.device)
            ops.scale_(loss.view(1), w)
            ops.scale_(dz, w)
            hdist.all_reduce_sum(loss)
        ctx.saved = dz
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ops.scale_(ctx.saved, dloss.contiguous()), None, None, None, None, None


class MocoLoss(nn.Module):
    """utils/losses.py:49-71.  ``memory_vectors`` is the device queue [K_pad, D] (K_pad = queue size rounded up to 16, extra rows zero
    and masked out) as held by models.moco.MemoryBank."""

    def __init__(self, normalize=True, temperature=1.0):
        super().__init__()
        self.normalize, self.temperature = normalize, temperature

    def forward(self, query, keys, memory_vectors, queue_size=None):
        k = memory_vectors.shape[0] if queue_size is None else queue_size
        return _MocoFn.apply(query, keys, memory_vectors, k, self.normalize, self.temperature)


class _ProtoNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, protos, inv_phi, labels, seg_end, module):
        # the prototypes carry no gradient: one call gives the loss and d loss / dq (csrc/protonce.hip); backward only scales, as in _MocoFn
        d = query.shape[1]
        qn, inv_q = ops.l2norm_fwd(query.detach().contiguous(), module.normalize)
        loss, module.last_lse, dq, module.last_flag = ops.proto_nce(qn, protos, inv_phi, labels, seg_end)
        ctx.saved = ops.l2norm_bwd(qn, inv_q, dq, d, module.normalize)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ops.scale_(ctx.saved, dloss.contiguous()), None, None, None, None, None


class ProtoNceLoss(nn.Module):
    """The ProtoNCE term of Prototypical Contrastive Learning (Li et al., ICLR 2021; not in the reference) without sampled negatives: the mean over the
    clusterings ("segments" of ``protos`` [ktot, D], cut by the python ints ``seg_end``) of the cross-entropy of softmax((q . c_j) / phi_j) against the query's
    own prototype, q the L2-normalised ``query`` [B, D], ``inv_phi`` [ktot] = 1 / phi, ``labels`` [segs, B] int32 indices inside each segment.  Gradients reach
    ``query`` only.  D % 4 == 0 (a multiple of 32 up to 128 takes the fused kernel).  ``last_flag`` (device int32 [1]; ops.check_proto_nce_flag) and ``last_lse``
    belong to the last forward: the flag is NOT read here - a trainer reads it once per epoch."""

    def __init__(self, normalize=True):
        super().__init__()
        self.normalize = bool(normalize)
        self.last_flag = self.last_lse = None

    def forward(self, query, protos, inv_phi, labels, seg_end):
        if query.dim() != 2 or protos.dim() != 2 or protos.shape[1] != query.shape[1] or query.shape[1] % 4 or query.shape[0] > _lib.PROTO_NCE_MAX_M:
            raise ValueError(f"ProtoNceLoss needs query [B, D] and protos [ktot, D] with D % 4 == 0 and B <= {_lib.PROTO_NCE_MAX_M}, got {tuple(query.shape)} and {tuple(protos.shape)}")
        if hdist.is_on():
            raise NotImplementedError("ProtoNceLoss is single-process: the prototypes are not replicated across ranks")
        return _ProtoNceFn.apply(query, protos, inv_phi, labels, tuple(int(e) for e in seg_end), self)


class _DenseNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, query, keys, pos, bank, queue_size, module):
        # keys and the queue carry no gradient: one call gives the loss and d loss / dq (csrc/densecl.hip); backward only scales, as in _MocoFn
        d = query.shape[1]
        qn, inv_q = ops.l2norm_fwd(query.detach().contiguous(), module.normalize)
        kn, _ = ops.l2norm_fwd(keys.detach().contiguous(), module.normalize)
        loss, module.last_lse, dq, module.last_flag = ops.queue_nce(qn, kn, pos, bank, queue_size, 1.0 / float(module.temperature))
        ctx.saved = ops.l2norm_bwd(qn, inv_q, dq, d, module.normalize)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return ops.scale_(ctx.saved, dloss.contiguous()), None, None, None, None, None


class DenseNceLoss(nn.Module):
    """The dense term of DenseCL (Wang et al., CVPR 2021; not in the reference): InfoNCE of every cell's embedding ``query`` [M, D] against the dense queue
    ``memory_vectors`` [>= queue_size, D], the positive of cell i being row ``pos[i]`` (int32, from ops.dense_match) of ``keys`` [Mk, D].  Both grids are
    L2-normalised here (``normalize``); gradients reach ``query`` only.  D % 4 == 0 (a multiple of 32 up to 128 takes the fused kernel), M <= 131072.
    ``last_flag`` (device int32 [1]; ops.check_queue_nce_flag) and ``last_lse`` belong to the last forward: the flag is NOT read here - a trainer reads it once
    per epoch."""

    def __init__(self, normalize=True, temperature=1.0):
        super().__init__()
        self.normalize, self.temperature = bool(normalize), float(temperature)
        self.last_flag = self.last_lse = None

    def forward(self, query, keys, pos, memory_vectors, queue_size=None):
        if (query.dim() != 2 or keys.dim() != 2 or memory_vectors.dim() != 2 or keys.shape[1] != query.shape[1] or memory_vectors.shape[1] != query.shape[1]
                or query.shape[1] % 4 or not 1 <= query.shape[0] <= _lib.QUEUE_NCE_MAX_M or pos.dim() != 1 or pos.shape[0] != query.shape[0]):
            raise ValueError(f"DenseNceLoss needs query [M, D], keys [Mk, D], a queue [K, D] and pos [M] with D % 4 == 0 and M <= {_lib.QUEUE_NCE_MAX_M}, got "
                             f"{tuple(query.shape)}, {tuple(keys.shape)}, {tuple(memory_vectors.shape)} and {tuple(pos.shape)}")
        if not self.temperature > 0.0:
            raise ValueError(f"DenseNceLoss needs a positive temperature (got {self.temperature})")
        if hdist.is_on():
            raise NotImplementedError("DenseNceLoss is single-process: the dense queue is not replicated across ranks")
        k = memory_vectors.shape[0] if queue_size is None else int(queue_size)
        return _DenseNceFn.apply(query, keys, pos, memory_vectors, k, self)


class _PirlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_features, patch_features, bank, pos_index, neg_index, module):
        # one launch sequence gives the loss and both gradients (the negatives' logits are bank-row products: constants); backward only scales them
        loss, dimg, dpatch, module.last_flag = ops.pirl_loss(bank, pos_index, neg_index, img_features.detach().contiguous(), patch_features.detach().contiguous(),
                                                             module.normalize, 1.0 / float(module.temp), module.loss_weight)
        ctx.saved = (dimg, dpatch)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dimg, dpatch = ctx.saved
        g = dloss.contiguous()
        return ops.scale_(dimg, g), ops.scale_(dpatch, g), None, None, None, None


class PirlLoss(nn.Module):
    """utils/losses.py:92-117 against the DEVICE memory bank: instead of the gathered positive / negative rows, ``forward`` takes the bank [N, D] and the
    int64 index vectors (``pos_index`` [B]: the batch's own rows, ``neg_index`` [K]) - the rows are gathered inside the loss kernel.  An index outside the
    bank raises SsvError: at once (``check=True``, one host synchronisation), or when the caller hands ``last_flag`` to ops.check_pirl_flag."""

    def __init__(self, normalize=True, temperature=1.0, loss_weight=0.5):
        super().__init__()
        self.loss_weight, self.normalize, self.temp = loss_weight, normalize, temperature
        self.last_flag = None

    def forward(self, img_features, patch_features, bank, pos_index, neg_index, check=True):
        if hdist.is_on():
            raise NotImplementedError("PirlLoss is single-process: the memory bank is not replicated across ranks")
        loss = _PirlFn.apply(img_features, patch_features, bank, pos_index, neg_index, self)
        if check:
            ops.check_pirl_flag(self.last_flag)
        return loss
