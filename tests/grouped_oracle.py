"""GPU-free restatement of the group-aware index arithmetic of csrc/conv_mfma.hip: group_span with the tiles and k-steps of fwd_tile / dgrad_tile as
the grouped launches take them, plan_wgrad with wgrad_row_split, and the skip rule of conv_wgrad_k.  tests/test_gpu_grouped_forms.py derives from it which
output columns a poisoned group may reach and which weight-gradient tiles stay unwritten; tests/test_grouped_forms_cpu.py ties it to the library
(ssv_conv2d_wgrad_grouped_workspace_bytes is host code) and shows that every case of the table reaches what its label claims.

A geometry is (N, H, W, C, K, R(=S), stride, pad, groups)."""
import torch
import torch.nn.functional as F


def cdiv(a, b):
    return -(-a // b)


def out_hw(geom):
    n, h, w, c, k, r, s, pad, g = geom
    return (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1


def group_span(n0, n1, og, ig, bk, ctot):
    """conv_mfma.hip:group_span - [lo, hi) of the contraction channels (whole k-steps, hi capped) that the output columns [n0, n1) see."""
    glo, ghi = n0 // og, (n1 - 1) // og
    return glo * ig // bk * bk, min(ctot, ((ghi + 1) * ig + bk - 1) // bk * bk)


def fwd_spans(c, k, groups):
    """[(n0, n1, lo, hi)] per column tile of ssv_conv2d_fwd_grouped on C input and K output channels, or None where the launch ignores the groups: groups == 1,
    the C == 4 tap-vector gather and the scalar gather (C % 16 != 0)."""
    if groups <= 1 or c == 4 or c % 16 != 0:
        return None
    bk = 32 if c % 32 == 0 else 16
    cg, kg = c // groups, k // groups
    return [(n0, min(n0 + 64, k)) + group_span(n0, min(n0 + 64, k), kg, cg, bk, c) for n0 in range(0, k, 64)]


def dgrad_spans(c, k, groups):
    """[(n0, n1, lo, hi)] per 64-column tile of ssv_conv2d_dgrad_grouped: columns are input channels, the contraction runs over the output channels."""
    if groups <= 1:
        return None
    bk = 32 if k % 32 == 0 else 16
    cg, kg = c // groups, k // groups
    return [(n0, min(n0 + 64, c)) + group_span(n0, min(n0 + 64, c), cg, kg, bk, k) for n0 in range(0, c, 64)]


def case_spans(entry, geom):
    """The spans of a case of tests/test_gpu_grouped_forms.py: (columns, contraction channels, spans)."""
    n, h, w, c, k, r, s, pad, g = geom
    if entry == "gfwd":
        return k, c, fwd_spans(c, k, g)
    if entry == "gdgrad_s1":                      # the forward kernel on the transposed bank: input and output channels change places
        return c, k, fwd_spans(k, c, g)
    assert entry == "gdgrad"
    return c, k, dgrad_spans(c, k, g)


def clean_columns(entry, geom, poisoned_group):
    """bool [columns]: True where the column's tile never stages the contraction channels of ``poisoned_group``."""
    ncol, nctr, spans = case_spans(entry, geom)
    per = nctr // geom[8]
    p0, p1 = poisoned_group * per, (poisoned_group + 1) * per
    clean = torch.zeros(ncol, dtype=torch.bool)
    for n0, n1, lo, hi in spans:
        clean[n0:n1] = hi <= p0 or p1 <= lo
    return clean


class WgradPlan:
    """conv_mfma.hip:plan_wgrad + wgrad_row_split for ssv_conv2d_wgrad_grouped; bn_kernel is the column tile the launch takes (wgrad_impl: 128 on the scalar
    gather, where the plan's 64 means one column tile either way)."""

    def __init__(self, geom):
        n, h, w, c, k, r, s, pad, g = geom
        ho, wo = out_hw(geom)
        self.m, self.rsc = n * ho * wo, r * r * c
        self.bd = g > 1 and c % 64 == 0
        self.bm = 128 if (k >= 128 and not self.bd) else 64
        self.bn = 64 if (self.rsc <= 64 or self.bd) else 128
        self.it, self.jt = cdiv(k, self.bm), cdiv(self.rsc, self.bn)
        tiles = self.it * self.jt
        if self.bd:
            cg, kg = c // g, k // g
            per_row = cdiv((cdiv(self.bm, kg) + 1) * cg, self.bn) + 1
            tiles = self.it * r * r * min(per_row, c // self.bn)
        ns = max(1, min((768 if self.bm == 128 else 1024) // tiles, cdiv(self.m, 256)))
        self.chunk = cdiv(cdiv(self.m, ns), 32) * 32
        self.nsplit = cdiv(self.m, self.chunk)
        self.bn_kernel = self.bn if c % 4 == 0 else 128
        self.workspace_bytes = self.nsplit * k * self.rsc * 4
        self.gather = "lin" if (r == 1 and pad == 0 and s == 1) else ("s1" if (s == 1 and (ho, wo) == (h, w) and 32 // wo + 1 <= ho) else "generic")
        self.chunks = [min(self.chunk, self.m - i * self.chunk) for i in range(self.nsplit)]


def wgrad_tiles(geom):
    """[(i0, i1, j0, j1, skipped)] over the [K][R*S*C] weight-gradient matrix: the tiles of the launch and conv_wgrad_k's skip rule."""
    n, h, w, c, k, r, s, pad, g = geom
    p = WgradPlan(geom)
    cg, kg = c // g, k // g
    out = []
    for i0 in range(0, k, p.bm):
        for j0 in range(0, p.rsc, p.bn_kernel):
            i1, j1 = min(i0 + p.bm, k), min(j0 + p.bn_kernel, p.rsc)
            skipped = False
            if g > 1 and j0 // c == (j1 - 1) // c:                # the column tile lies inside one tap
                c0 = j0 % c
                c1 = c0 + (j1 - j0)
                skipped = (i1 - 1) // kg < c0 // cg or (c1 - 1) // cg < i0 // kg
            out.append((i0, i1, j0, j1, skipped))
    return out


def skipped_mask(geom):
    """bool [K][R][S][C]: True on the entries of tiles that conv_wgrad_k returns from without writing."""
    n, h, w, c, k, r, s, pad, g = geom
    mask = torch.zeros(k, r * r * c, dtype=torch.bool)
    for i0, i1, j0, j1, skipped in wgrad_tiles(geom):
        mask[i0:i1, j0:j1] = skipped
    return mask.view(k, r, r, c)


def diagonal_mask(geom):
    """bool [K][R][S][C]: True on the diagonal blocks of the bank, the entries ssv_group_extract reads."""
    n, h, w, c, k, r, s, pad, g = geom
    kk, cc = torch.arange(k) // (k // g), torch.arange(c) // (c // g)
    return (kk[:, None] == cc[None, :])[:, None, None, :].expand(k, r, r, c)


# ------------------------------------------------------------------------------------------------------------------- fp64 references (NHWC / OHWI)
def expand_bank(wg, groups):
    """[K][R][S][C/groups] -> the dense block-diagonal [K][R][S][C] (ssv_group_expand), in the dtype of wg."""
    k, r, s, cg = wg.shape
    kg = k // groups
    wd = torch.zeros(k, r, s, cg * groups, dtype=wg.dtype)
    for g in range(groups):
        wd[g * kg:(g + 1) * kg, :, :, g * cg:(g + 1) * cg] = wg[g * kg:(g + 1) * kg]
    return wd


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv64(x, wg, stride, pad, groups):
    """x [N][H][W][C], wg [K][R][S][C/groups] -> y [N][Ho][Wo][K] (F.conv2d with groups)."""
    return F.conv2d(_nchw(x), _nchw(wg), stride=stride, padding=pad, groups=groups).permute(0, 2, 3, 1)


def dgrad64(dy, wg, xshape, stride, pad, groups):
    n, h, w, c = xshape
    return torch.nn.grad.conv2d_input((n, c, h, w), _nchw(wg), _nchw(dy), stride=stride, padding=pad, groups=groups).permute(0, 2, 3, 1)


def wgrad64(x, dy, wgshape, stride, pad, groups):
    """-> [K][R][S][C/groups], the grouped filter's gradient."""
    k, r, s, cg = wgshape
    return torch.nn.grad.conv2d_weight(_nchw(x), (k, cg, r, s), _nchw(dy), stride=stride, padding=pad, groups=groups).permute(0, 2, 3, 1)
