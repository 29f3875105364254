"""TEST INFRASTRUCTURE - CPU restatement (torch, any float dtype) of every STAGE of the two Winograd families (csrc/winograd.hip, csrc/winograd44.hip), pinned to
F.conv2d / F.conv_transpose2d / torch.nn.grad.conv2d_weight in float64 by tests/test_wino_oracle_cpu.py and used as the reference of tests/test_gpu_wino_forms.py
(float64 = ref64, float32 = ref32).

Matrices, from the header comments of the two kernel files:
  F(2x2, 3x3)   B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]]   G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]]   A^T = [[1,1,1,0],[0,1,-1,-1]]
  F(4x4, 3x3)   the B^T (6x6), G (6x3), A^T (4x6) of the points {0, 1, -1, 1/2, -2, inf}
Layouts, the headers': U [P][K][C]; V, M, dM [P][T][channels] with position p = xi * (4 | 6) + nu; tiles in (n, i, j) order, T = N * ceil(H/t) * ceil(W/t) (t = 2 | 4); the
input is zero outside the image (padding 1); output pixels past the edge are dropped and are zero in the dY transforms.

Every stage is written in the ORDER OF OPERATIONS OF ITS KERNEL (the rows of B^T, A, A^T, G as the kernels spell them, left to right, first pass along xi then along nu), so
that the float32 evaluation of a stage that only adds and halves - all of F(2x2) except the partial sums - has the kernel's bits; `matrices(fam)` gives the same
transforms as plain matrices, and the CPU test holds the two forms to each other.

Groups of the output transforms' partials (`group_rows`), as the kernel headers state them: F(2x2) 16 consecutive tiles (the last group short when T % 16 != 0); F(4x4) one
row of tiles of one image, and for the statistics of a map with H % 4 != 0 one image.
"""
import torch

F22, F44 = 22, 44
TILE = {F22: 2, F44: 4}
POS = {F22: 4, F44: 6}                                                    # positions per axis: P = POS ** 2
WG_TILES = 16                                                             # tiles per workgroup of wino_output_k


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- the library's host answers, restated
def tile_grid(fam, h, w):
    return cdiv(h, TILE[fam]), cdiv(w, TILE[fam])


def tiles(fam, n, h, w):
    """ssv_wino_tiles / ssv_wino44_tiles"""
    if n <= 0 or h <= 0 or w <= 0:
        return 0
    th, tw = tile_grid(fam, h, w)
    return n * th * tw


def groups(fam, n, h, w, stats=False):
    """ssv_wino_groups(N, H, W) / ssv_wino44_groups(N, H, W, stats)"""
    if n <= 0 or h <= 0 or w <= 0:
        return 0
    if fam == F22:
        return cdiv(tiles(F22, n, h, w), WG_TILES)
    return n * cdiv(h, 4) if (not stats or h % 4 == 0) else n


def stats_rows_per_group(fam, n, h, w):
    """ssv_wino_stats_rows_per_group (0: the map does not partition evenly) / ssv_wino44_stats_rows_per_group"""
    if n <= 0 or h <= 0 or w <= 0:
        return 0
    if fam == F44:
        return 4 * w if h % 4 == 0 else h * w
    if h % 2 == 0 and w % 2 == 0:
        return 4 * WG_TILES
    return h * w if cdiv(h, 2) * cdiv(w, 2) == WG_TILES else 0


def group_rows(fam, n, h, w, stats=False):
    """For every group, the rows (pixel indices into the [N * H * W] rows of y, ascending) its partial summarises."""
    t = TILE[fam]
    th, tw = tile_grid(fam, h, w)
    pix = torch.arange(n * h * w).reshape(n, h, w)

    def of_tile(q):
        img, r = divmod(q, th * tw)
        i, j = divmod(r, tw)
        return pix[img, t * i:min(t * i + t, h), t * j:min(t * j + t, w)].reshape(-1)

    total = n * th * tw
    if fam == F22:
        runs = [range(g * WG_TILES, min((g + 1) * WG_TILES, total)) for g in range(cdiv(total, WG_TILES))]
    elif not stats or h % 4 == 0:
        runs = [range(g * tw, (g + 1) * tw) for g in range(n * th)]
    else:
        runs = [range(g * th * tw, (g + 1) * th * tw) for g in range(n)]
    return [torch.cat([of_tile(q) for q in run]).sort().values for run in runs]


# ------------------------------------------------------------------------------------------- the transforms as matrices
def matrices(fam, dt=torch.float64):
    """(B^T, G, A^T) of the family"""
    if fam == F22:
        bt = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
        g = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
        at = [[1, 1, 1, 0], [0, 1, -1, -1]]
    else:
        bt = [[1, -1.5, -2, 1.5, 1, 0], [0, -1, .5, 2.5, 1, 0], [0, 1, -2.5, .5, 1, 0], [0, -2, -1, 2, 1, 0], [0, .5, -1, -.5, 1, 0], [0, 1, -1.5, -2, 1.5, 1]]
        g = [[1, 0, 0], [1 / 3, 1 / 3, 1 / 3], [-1 / 3, 1 / 3, -1 / 3], [-16 / 15, -8 / 15, -4 / 15], [1 / 15, -2 / 15, 4 / 15], [0, 0, 1]]
        at = [[1, 1, 1, 1, 1, 0], [0, 1, -1, .5, -2, 0], [0, 1, 1, .25, 4, 0], [0, 1, -1, .125, -8, 1]]
    return tuple(torch.tensor(m, dtype=torch.float64).to(dt) for m in (bt, g, at))


# ------------------------------------------------------------------------------------------- one-dimensional transforms, in the kernels' order
def _c(v, like):
    """a constant as the kernel's float literal (1.f / 3.f is the correctly rounded third in either width)"""
    return torch.tensor(v, dtype=torch.float64).to(like.dtype)


def _bt(fam, d):
    if fam == F22:                                                        # wino_input_k
        return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    return [d[0] - 1.5 * d[1] - 2.0 * d[2] + 1.5 * d[3] + d[4],           # bt6
            -d[1] + 0.5 * d[2] + 2.5 * d[3] + d[4],
            d[1] - 2.5 * d[2] + 0.5 * d[3] + d[4],
            -2.0 * d[1] - d[2] + 2.0 * d[3] + d[4],
            0.5 * d[1] - d[2] - 0.5 * d[3] + d[4],
            d[1] - 1.5 * d[2] - 2.0 * d[3] + 1.5 * d[4] + d[5]]


def _at(fam, m):
    if fam == F22:                                                        # wino_output_k
        return [m[0] + m[1] + m[2], m[1] - m[2] - m[3]]
    return [m[0] + m[1] + m[2] + m[3] + m[4],                             # at6
            m[1] - m[2] + 0.5 * m[3] - 2.0 * m[4],
            m[1] + m[2] + 0.25 * m[3] + 4.0 * m[4],
            m[1] - m[2] + 0.125 * m[3] - 8.0 * m[4] + m[5]]


def _a(fam, y):
    if fam == F22:                                                        # wino_dy_k
        return [y[0], y[0] + y[1], y[0] - y[1], -y[1]]
    return [y[0],                                                         # a6
            y[0] + y[1] + y[2] + y[3],
            y[0] - y[1] + y[2] - y[3],
            y[0] + 0.5 * y[1] + 0.25 * y[2] + 0.125 * y[3],
            y[0] - 2.0 * y[1] + 4.0 * y[2] - 8.0 * y[3],
            y[3]]


def _g(fam, g):
    if fam == F22:                                                        # wino_filter_k
        return [g[0], 0.5 * (g[0] + g[1] + g[2]), 0.5 * (g[0] - g[1] + g[2]), g[2]]
    third, fif = _c(1 / 3, g[0]), _c(1 / 15, g[0])                        # g3
    return [g[0], (g[0] + g[1] + g[2]) * third, (-g[0] + g[1] - g[2]) * third,
            (-16.0 * g[0] - 8.0 * g[1] - 4.0 * g[2]) * fif, (g[0] - 2.0 * g[1] + 4.0 * g[2]) * fif, g[2]]


def _gt(fam, u):
    if fam == F22:                                                        # wino_dfilter_k
        return [u[0] + 0.5 * (u[1] + u[2]), 0.5 * (u[1] - u[2]), 0.5 * (u[1] + u[2]) + u[3]]
    third, fif = _c(1 / 3, u[0]), _c(1 / 15, u[0])                        # gt3
    return [u[0] + (u[1] - u[2]) * third + (u[4] - 16.0 * u[3]) * fif,
            (u[1] + u[2]) * third - (8.0 * u[3] + 2.0 * u[4]) * fif,
            (u[1] - u[2]) * third + (4.0 * u[4] - 4.0 * u[3]) * fif + u[5]]


def _two_pass(f, fam, x):
    """x [..., a, b, ch]: f along a (for every b), then along b - the order of every kernel of both files.  -> [..., a', b', ch]"""
    rows = torch.stack(f(fam, list(x.unbind(-3))), dim=-3)
    return torch.stack(f(fam, list(rows.unbind(-2))), dim=-2)


def _to_positions(x):
    """[T, a, b, ch] -> [a * b][T][ch]"""
    t, a, b, ch = x.shape
    return x.permute(1, 2, 0, 3).reshape(a * b, t, ch).contiguous()


# ------------------------------------------------------------------------------------------- the stages
def filter_transform(fam, w, dt):
    """w [K][3][3][C] (OHWI) -> U [P][K][C] = G g G^T"""
    g = w.to(dt).permute(0, 3, 1, 2).unsqueeze(-1)                        # [K, C, r, s, 1]
    u = _two_pass(_g, fam, g)                                             # [K, C, xi, nu, 1]
    k, c = w.shape[0], w.shape[3]
    return u.reshape(k, c, -1).permute(2, 0, 1).contiguous()


def filter_grad(fam, du, dt, prior=None):
    """dU [P][K][C] -> dg [K][3][3][C] = G^T dU G (+ prior [K][3][3][C]: the accumulating form)"""
    p, k, c = du.shape
    u = du.to(dt).permute(1, 2, 0).reshape(k, c, POS[fam], POS[fam], 1)
    dg = _two_pass(_gt, fam, u).reshape(k, c, 3, 3).permute(0, 2, 3, 1).contiguous()
    return dg if prior is None else prior.to(dt) + dg


def relu_affine(x, scale, shift, dt):
    """relu(x * scale + shift) in dt: what the fused input transforms (and ssv_bn_apply) form per element"""
    return (x.to(dt) * scale.to(dt) + shift.to(dt)).clamp_min(0.0)


def _patches(fam, x, halo):
    """x [N][H][W][ch] -> [T][t + 2 halo][t + 2 halo][ch]: the tile's pixels with `halo` pixels around it, zero outside the image"""
    t = TILE[fam]
    n, h, w, ch = x.shape
    th, tw = tile_grid(fam, h, w)
    xp = torch.zeros((n, th * t + 2 * halo, tw * t + 2 * halo, ch), dtype=x.dtype)
    xp[:, halo:halo + h, halo:halo + w] = x
    p = xp.unfold(1, t + 2 * halo, t).unfold(2, t + 2 * halo, t)          # [N, th, tw, ch, a, b]
    return p.permute(0, 1, 2, 4, 5, 3).reshape(n * th * tw, t + 2 * halo, t + 2 * halo, ch)


def input_transform(fam, x, dt, scale=None, shift=None):
    """x [N][H][W][C] (+ the producer's BatchNorm + ReLU) -> V [P][T][C] = B^T d B"""
    a = x.to(dt) if scale is None else relu_affine(x, scale, shift, dt)
    return _to_positions(_two_pass(_bt, fam, _patches(fam, a, 1)))


def dy_transform(fam, dy, dt):
    """dy [N][H][W][K] -> dM [P][T][K] = A dY A^T"""
    return _to_positions(_two_pass(_a, fam, _patches(fam, dy.to(dt), 0)))


def output_transform(fam, m, n, h, w, dt):
    """M [P][T][K] -> y [N][H][W][K] = A^T M A, the pixels past the edge dropped"""
    t = TILE[fam]
    th, tw = tile_grid(fam, h, w)
    p, tt, k = m.shape
    assert p == POS[fam] ** 2 and tt == n * th * tw
    y = _two_pass(_at, fam, m.to(dt).reshape(POS[fam], POS[fam], tt, k).permute(2, 0, 1, 3))      # [T, t, t, K]
    y = y.reshape(n, th, tw, t, t, k).permute(0, 1, 3, 2, 4, 5).reshape(n, th * t, tw * t, k)
    return y[:, :h, :w].contiguous()


def stats_partials(fam, y, dt):
    """(pmean, pm2) [groups][K] of y [N][H][W][K]: per group mean and centred sum of squares"""
    n, h, w, k = y.shape
    rows = y.to(dt).reshape(-1, k)
    mean = torch.stack([rows[r].mean(0) for r in group_rows(fam, n, h, w, True)])
    m2 = torch.stack([((rows[r] - rows[r].mean(0)) ** 2).sum(0) for r in group_rows(fam, n, h, w, True)])
    return mean, m2


def gate_bit(x, scale, shift):
    """the ReLU bit of the gated output transforms: the sign of the kernel's fmaf, decided in float64 (exact product, one rounding: the same sign)"""
    return x.double() * scale.double() + shift.double() > 0


def pack_mask(bit):
    """one byte per four channels, bit e = element e positive (ssv_bn_apply's byte mask)"""
    b = bit.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def gated(fam, y, bit, x, mean, invstd, dt):
    """g = bit ? y : 0 and its partial sums (sum g, sum g * xhat) [groups][K], xhat = (x - mean) * invstd"""
    n, h, w, k = y.shape
    g = torch.where(bit, y.to(dt), torch.zeros((), dtype=dt))
    gx = g * ((x.to(dt) - mean.to(dt)) * invstd.to(dt))
    rows = group_rows(fam, n, h, w, False)
    g2, gx2 = g.reshape(-1, k), gx.reshape(-1, k)
    return g, torch.stack([g2[r].sum(0) for r in rows]), torch.stack([gx2[r].sum(0) for r in rows])


def dyin(g, x, coef, dt):
    """the output gradient ssv_wino44_dy_transform_both forms on load: A g + (B (x - mean) + D), coef = [A | mean | B | D]"""
    a, mean, b, d = (coef[i].to(dt) for i in range(4))
    return g.to(dt) * a + ((x.to(dt) - mean) * b + d)


# ------------------------------------------------------------------------------------------- the chains (composition of the stages)
def gemm(v, u):
    """M_p [T][K] = V_p [T][C] . U_p^T [C][K]"""
    return torch.einsum("ptc,pkc->ptk", v, u)


def wgrad_gemm(dm, v):
    """dU_p [K][C] = dM_p^T [K][T] . V_p [T][C]"""
    return torch.einsum("ptk,ptc->pkc", dm, v)


def transposed_filter(w):
    """wt[c][2 - r][2 - s][k] = w[k][r][s][c] (ssv_filter_transpose): the data gradient's filter"""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def conv_fwd(fam, x, w, dt):
    n, h, w_, _ = x.shape
    return output_transform(fam, gemm(input_transform(fam, x, dt), filter_transform(fam, w, dt)), n, h, w_, dt)


def conv_dgrad(fam, dy, w, dt):
    return conv_fwd(fam, dy, transposed_filter(w), dt)


def conv_wgrad(fam, x, dy, dt):
    return filter_grad(fam, wgrad_gemm(dy_transform(fam, dy, dt), input_transform(fam, x, dt)), dt)
