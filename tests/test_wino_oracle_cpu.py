"""CPU: the torch restatement of the Winograd stages (tests/wino_oracle.py) is proven here, not the kernels: composed in float64 the stages equal F.conv2d,
F.conv_transpose2d and torch.nn.grad.conv2d_weight to 1e-12 relative, for both families, on whole, ragged and sub-tile maps; each stage written in its kernel's order of
operations equals the same transform as a plain matrix product; the group partition is a partition; and the host answers the oracle restates (tiles, groups, rows per
statistics group) are the library's own, which need no GPU."""
import pytest
import torch
import torch.nn.functional as F

import wino_oracle as wo

MAPS = ((8, 8), (7, 7), (9, 5), (3, 2), (4, 4), (12, 12))
FAMS = (wo.F22, wo.F44)
D = torch.float64


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _case(h, w, n=2, c=5, k=3):
    g = torch.Generator().manual_seed(1000 * h + w)
    x = torch.randn(n, h, w, c, generator=g, dtype=D)
    wt = torch.randn(k, 3, 3, c, generator=g, dtype=D)                   # OHWI
    dy = torch.randn(n, h, w, k, generator=g, dtype=D)
    return x, wt, dy


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("h,w", MAPS)
def test_composed_stages_equal_the_fp64_convolutions(fam, h, w):
    x, wt, dy = _case(h, w)
    xn, wn, dyn = x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    fwd = F.conv2d(xn, wn, padding=1).permute(0, 2, 3, 1)
    assert _rel(wo.conv_fwd(fam, x, wt, D), fwd) <= 1e-12
    dgrad = F.conv_transpose2d(dyn, wn, padding=1).permute(0, 2, 3, 1)
    assert _rel(wo.conv_dgrad(fam, dy, wt, D), dgrad) <= 1e-12
    wgrad = torch.nn.grad.conv2d_weight(xn, wn.shape, dyn, padding=1).permute(0, 2, 3, 1)
    assert _rel(wo.conv_wgrad(fam, x, dy, D), wgrad) <= 1e-12
    # the accumulating filter gradient is prior + overwrite; the fused input is the transform of the materialised activation
    prior = torch.randn(wt.shape, generator=torch.Generator().manual_seed(3), dtype=D)
    du = wo.wgrad_gemm(wo.dy_transform(fam, dy, D), wo.input_transform(fam, x, D))
    assert torch.equal(wo.filter_grad(fam, du, D, prior=prior), prior + wo.filter_grad(fam, du, D))
    sc, sh = torch.rand(x.shape[3], dtype=D) + 0.5, torch.randn(x.shape[3], dtype=D) * 0.3
    assert torch.equal(wo.input_transform(fam, x, D, sc, sh), wo.input_transform(fam, torch.relu(x * sc + sh), D))


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("h,w", MAPS)
def test_kernel_order_stages_equal_the_matrix_forms(fam, h, w):
    """B^T d B, A dY A^T, A^T M A, G g G^T and G^T dU G as einsums with the matrices of the header comments"""
    x, wt, dy = _case(h, w)
    bt, g, at = wo.matrices(fam)
    n, c, k, t, p = x.shape[0], x.shape[3], wt.shape[0], wo.TILE[fam], wo.POS[fam]
    th, tw = wo.tile_grid(fam, h, w)
    assert bt.shape == (p, p) and g.shape == (p, 3) and at.shape == (t, p)
    xp = torch.zeros(n, th * t + 2, tw * t + 2, c, dtype=D)
    xp[:, 1:h + 1, 1:w + 1] = x
    yp = torch.zeros(n, th * t, tw * t, k, dtype=D)
    yp[:, :h, :w] = dy
    v = wo.input_transform(fam, x, D)
    dm = wo.dy_transform(fam, dy, D)
    assert v.shape == (p * p, wo.tiles(fam, n, h, w), c) and dm.shape == (p * p, wo.tiles(fam, n, h, w), k)
    for img in range(n):
        for i in range(th):
            for j in range(tw):
                q = (img * th + i) * tw + j
                d = xp[img, t * i:t * i + t + 2, t * j:t * j + t + 2]                      # [a, b, c]
                ref = torch.einsum("xa,abc,nb->xnc", bt, d, bt).reshape(p * p, c)
                assert _rel(v[:, q], ref) <= 1e-14 if float(ref.norm()) else not v[:, q].any()
                ref = torch.einsum("ax,abk,bn->xnk", at, yp[img, t * i:t * i + t, t * j:t * j + t], at).reshape(p * p, k)
                assert _rel(dm[:, q], ref) <= 1e-14
    u = wo.filter_transform(fam, wt, D)
    assert _rel(u, torch.einsum("xr,krsc,ns->xnkc", g, wt, g).reshape(p * p, k, c)) <= 1e-14
    du = torch.randn(p * p, k, c, generator=torch.Generator().manual_seed(5), dtype=D)
    assert _rel(wo.filter_grad(fam, du, D), torch.einsum("xr,xnkc,ns->krsc", g, du.reshape(p, p, k, c), g)) <= 1e-14
    m = torch.randn(p * p, wo.tiles(fam, n, h, w), k, generator=torch.Generator().manual_seed(6), dtype=D)
    full = torch.einsum("ax,xnqk,bn->qabk", at, m.reshape(p, p, -1, k), at)                  # [T, t, t, K]
    full = full.reshape(n, th, tw, t, t, k).permute(0, 1, 3, 2, 4, 5).reshape(n, th * t, tw * t, k)[:, :h, :w]
    assert _rel(wo.output_transform(fam, m, n, h, w, D), full) <= 1e-14


def test_f22_stages_are_exact_in_float32():
    """adds and halves only: the float32 evaluation of F(2x2)'s transforms of small integers is the float64 one"""
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-64, 64, (2, 7, 5, 4), generator=g).float()
    w = torch.randint(-64, 64, (3, 3, 3, 4), generator=g).float()
    for f32, f64 in ((wo.input_transform(wo.F22, x, torch.float32), wo.input_transform(wo.F22, x, D)),
                     (wo.dy_transform(wo.F22, x, torch.float32), wo.dy_transform(wo.F22, x, D)),
                     (wo.filter_transform(wo.F22, w, torch.float32), wo.filter_transform(wo.F22, w, D))):
        assert f32.dtype == torch.float32 and torch.equal(f32.double(), f64)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("stats", (False, True))
@pytest.mark.parametrize("n,h,w", [(2, 8, 8), (3, 7, 7), (3, 9, 5), (5, 3, 2), (2, 4, 4), (1, 12, 12), (2, 7, 8), (2, 8, 6), (2, 6, 5)])
def test_groups_partition_the_rows_as_the_headers_state(fam, stats, n, h, w):
    rows = wo.group_rows(fam, n, h, w, stats)
    assert len(rows) == wo.groups(fam, n, h, w, stats)
    allrows = torch.cat(rows)
    assert allrows.numel() == n * h * w and torch.equal(allrows.sort().values, torch.arange(n * h * w))        # every pixel in exactly one group
    rpg = wo.stats_rows_per_group(fam, n, h, w)
    if stats and rpg:
        # the statistics partials need equal groups - but for the last, which ssv_bn_stats_finalize takes short (F(2x2) on an even map with T % 16 != 0)
        assert all(r.numel() == rpg for r in rows[:-1]) and 0 < rows[-1].numel() <= rpg
        assert fam == wo.F22 or rows[-1].numel() == rpg
    if fam == wo.F22:
        t = wo.tiles(fam, n, h, w)
        assert len(rows) == wo.cdiv(t, 16) and (t % 16 == 0 or rows[-1].numel() < 64)
    elif not stats or h % 4 == 0:
        assert all(int(r.max()) - int(r.min()) < 4 * w for r in rows)    # one row of tiles: at most 4 image rows
    else:
        assert all(torch.equal(r, torch.arange(g * h * w, (g + 1) * h * w)) for g, r in enumerate(rows))


def test_partials_and_gate_sum_to_the_whole():
    g = torch.Generator().manual_seed(4)
    for fam in FAMS:
        for n, h, w in ((3, 7, 7), (2, 8, 6), (3, 9, 5), (3, 4, 4)):
            y = torch.randn(n, h, w, 4, generator=g, dtype=D)
            x = torch.randn(n, h, w, 4, generator=g, dtype=D)
            sc, sh = torch.rand(4, dtype=D) + 0.5, torch.randn(4, dtype=D) * 0.3
            mean, invstd = x.reshape(-1, 4).mean(0), 1.0 / x.reshape(-1, 4).std(0)
            bit = wo.gate_bit(x, sc, sh)
            assert torch.equal(bit, x * sc + sh > 0)
            gy, sg, sgx = wo.gated(fam, y, bit, x, mean, invstd, D)
            assert torch.equal(gy, torch.where(bit, y, torch.zeros((), dtype=D)))
            assert _rel(sg.sum(0), gy.reshape(-1, 4).sum(0)) <= 1e-13
            assert _rel(sgx.sum(0), (gy * ((x - mean) * invstd)).reshape(-1, 4).sum(0)) <= 1e-13
            if wo.stats_rows_per_group(fam, n, h, w):
                pm, pm2 = wo.stats_partials(fam, y, D)
                cnt = torch.tensor([float(r.numel()) for r in wo.group_rows(fam, n, h, w, True)], dtype=D)[:, None]
                tot = y.reshape(-1, 4).mean(0)
                assert _rel((pm * cnt).sum(0) / cnt.sum(), tot) <= 1e-13  # the parallel-variance merge of the groups is the whole
                assert _rel(pm2.sum(0) + (cnt * (pm - tot) ** 2).sum(0), ((y.reshape(-1, 4) - tot) ** 2).sum(0)) <= 1e-13
    b = torch.tensor([[True, False, False, True], [False, True, True, False]])
    assert wo.pack_mask(b).tolist() == [9, 6]


def test_host_answers_are_the_librarys():
    from ssv_amd import _lib
    lib = _lib.load()
    shapes = [(n, h, w) for n in (1, 2, 3, 5) for h in (1, 2, 3, 4, 6, 7, 8, 9, 12, 14) for w in (1, 2, 5, 6, 7, 8, 12, 14)] + [(0, 4, 4), (2, 0, 4), (2, 4, -1)]
    for n, h, w in shapes:
        assert wo.tiles(wo.F22, n, h, w) == lib.ssv_wino_tiles(n, h, w)
        assert wo.tiles(wo.F44, n, h, w) == lib.ssv_wino44_tiles(n, h, w)
        assert wo.groups(wo.F22, n, h, w) == lib.ssv_wino_groups(n, h, w)
        assert wo.stats_rows_per_group(wo.F22, n, h, w) == lib.ssv_wino_stats_rows_per_group(n, h, w)
        assert wo.stats_rows_per_group(wo.F44, n, h, w) == lib.ssv_wino44_stats_rows_per_group(n, h, w)
        for stats in (0, 1):
            assert wo.groups(wo.F44, n, h, w, bool(stats)) == lib.ssv_wino44_groups(n, h, w, stats)
    assert wo.stats_rows_per_group(wo.F22, 2, 7, 7) == 49 and wo.stats_rows_per_group(wo.F22, 2, 9, 5) == 0 and wo.stats_rows_per_group(wo.F22, 2, 8, 6) == 64
