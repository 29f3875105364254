"""Every launch form of the group-aware conv entry points (csrc/conv_mfma.hip: ssv_conv2d_fwd_grouped, ssv_conv2d_dgrad_grouped, ssv_conv2d_wgrad_grouped with
ssv_conv2d_wgrad_grouped_workspace_bytes) against fp64 on the CPU, in BOTH arithmetics, straight through the C ABI (ops.conv2d_dgrad(groups=g) for the stride-1
data gradient only, where ops is the one caller that builds the transposed bank).

The operand is the DENSE block-diagonal bank of a grouped filter (grouped_oracle.expand_bank, what ssv_group_expand makes); references are F.conv2d(groups=g),
conv2d_input and conv2d_weight in fp64 on the GROUPED filter, the magnitude A the same operation on absolute values.  Helpers, TAU, the floor and GUARD are those
of tests/test_gpu_conv_forms.py, imported.  Every case runs under ops.arithmetic("f32") and under ops.arithmetic("bf16x3") and is held to that file's rules:

  (a) |got - ref| <= TAU * 2^-24 * A + floor (weight gradients: on the diagonal blocks, the entries ssv_group_extract reads);
  (b) where the bf16x3 form is "f32" the two runs are one launch and bit-identical - the strided data gradient also with planes attached to the descriptor, which
      dgrad_tile must ignore on a bank.  Where a bf16-piece kernel runs: contracted channels per group a multiple of 32 (forward Cg, stride-1 data gradient Kg) and
      every weight gradient keep tests/test_gpu_split.py's bar, bf16x3 relative l2 error <= 1.05 x the fp32-MFMA one + 1e-9; with fewer channels per group a 32-channel
      k-tile is mostly exact zeros - fp32 MFMA rounds only for its nonzero products, the six piece products round whatever the tile holds - and the bar is
      SPARSE_BANK_BAR, the worst measured ratio x 1.15 (the ratios: profiles/grouped_forms_report.json).  The depthwise forward (one channel per group, one
      accumulator) measures 2.035: a finding explained over SPARSE_BANK_BAR, reported, and held by (a) alone - no bar is set for it;
  (c) ssv_conv_arithmetic(desc, product) reports the case's form (the strided data gradient: on the descriptor ops builds for a bank, without planes);
  (e) every output is a view into a NaN-prefilled buffer with GUARD floats behind it: nothing inside left NaN, nothing behind written.  Weight-gradient banks
      instead: diagonal blocks finite, every entry of a tile that the restated skip rule skips NaN in dwd AND in every slab of the workspace (the test owns it:
      exactly ssv_conv2d_wgrad_grouped_workspace_bytes, NaN-filled, guarded), entries of worked tiles finite, both guards untouched;
  (f) the grouped forward and stride-1 data gradient == the dense entry point on the same bank bit for bit; the strided data gradient too wherever both run the
      same instruction (under f32 always, in both arithmetics when C < 128).

test_poisoned_group_stays_outside_the_span proves the span is honoured (a build that ignored the groups would pass (a)-(f)): one group's contracted channels
are NaN, every column whose tile's restated span (tests/grouped_oracle.py) excludes them stays finite and inside (a), and the dense entry point is non-finite there.
test_refusals: every refused call leaves its outputs at their prefill.

Branches (label, forms, the function of conv_mfma.hip that selects it) - tests/test_grouped_forms_cpu.py keeps CASES honest and shows per case that the restated
spans / plans reach what the label claims:

  gfwd.span_bk32           f32 sp1 sp2   conv_mfma.hip:group_span  forward, K-step 32: two 64-column tiles with disjoint spans (stride 1; stride 2 on an odd map)
  gfwd.spans_differ        f32 sp1 sp2   conv_mfma.hip:group_span  Cg != Kg (4 in / 8 out per group and the reverse)
  gfwd.straddle            f32 sp2       conv_mfma.hip:group_span  Kg = 96: the middle tile holds columns of both groups
  gfwd.k_ragged            f32 sp1       conv_mfma.hip:group_span  K = 132: the last tile is 4 columns of one group, lower edge 32
  gfwd.span_rounded        f32 sp1       conv_mfma.hip:group_span  Cg = 24: neither edge of the second span is a whole k-step before rounding
  gfwd.span_bk16           f32           conv_mfma.hip:launch_fwd  C % 32 != 0: K-step 16
  gfwd.1x1                 f32 sp1       conv_mfma.hip:launch_fwd  1x1 / no padding: the loader without bounds tests
  gfwd.taps5               f32 sp2       conv_mfma.hip:launch_fwd  5x5 / stride 2: 25 taps per channel chunk
  gfwd.depthwise           f32 sp1       conv_mfma.hip:group_span  Cg = Kg = 1
  gfwd.dense_scalar        f32           conv_mfma.hip:launch_fwd  C % 16 != 0: the scalar gather ignores the groups
  gfwd.dense_c4            f32           conv_mfma.hip:launch_fwd  C == 4: the tap-vector gather ignores the groups
  gfwd.groups1             f32 sp1       conv_mfma.hip:fwd_tile  groups == 1: ssv_conv2d_fwd's launch, wide tile included
  gdgrad.s1_as_fwd         f32 sp1 sp2   ops.py conv2d_dgrad  stride 1: ssv_conv2d_fwd_grouped on the transposed bank (Cg and Kg change places)
  gdgrad.bk32              f32           conv_mfma.hip:dgrad_tile  strided kernel, 256 x 64 tile, K-step 32, odd map
  gdgrad.bk16              f32           conv_mfma.hip:dgrad_tile  K % 32 != 0: K-step 16
  gdgrad.no_tap_classes    f32           conv_mfma.hip:dgrad_impl  1x1 / stride 2: three parity classes without a tap (addend / zeros)
  gdgrad.stride1_entry     f32           conv_mfma.hip:dgrad_impl  the strided kernel at stride 1
  gdgrad.stride3           f32           conv_mfma.hip:dgrad_impl  nine parity classes
  gdgrad.c_ragged          f32           conv_mfma.hip:group_span  C = 132: the last tile is 4 columns
  gwgrad.bd_s1             f32 sp1       conv_mfma.hip:plan_wgrad  block-diagonal plan (C % 64 == 0: 64 x 64 tiles), S1 gather
  gwgrad.bd_generic        f32 sp1       conv_mfma.hip:plan_wgrad  block-diagonal plan, generic gather (stride 2)
  gwgrad.bd_lin            f32 sp1       conv_mfma.hip:plan_wgrad  block-diagonal plan, LIN gather (1x1)
  gwgrad.bd_spans_differ   f32 sp1       conv_mfma.hip:plan_wgrad  block-diagonal plan, Cg != Kg, generic gather (5x5 map)
  gwgrad.dense_tiles_skip  f32 sp1       conv_mfma.hip:plan_wgrad  C % 64 != 0: 128 x 128 tiles, two of four skipped
  gwgrad.dense_tiles_noskip f32 sp1      conv_mfma.hip:plan_wgrad  C % 64 != 0, column tiles straddle taps: none skipped
  gwgrad.gbk               f32           conv_mfma.hip:wgrad_impl  C % 4 != 0: scalar gather, 128-column tile
  gwgrad.nsplit_ragged     f32 sp1       conv_mfma.hip:wgrad_row_split  three row chunks, the last one short; tiles skipped in every slab
  gwgrad.accumulate        f32 sp1       conv_mfma.hip:wgrad_impl  dwd += on a nonzero prior
  gwgrad.depthwise         f32 sp1       conv_mfma.hip:plan_wgrad  Cg = Kg = 1, block-diagonal plan
"""
import ctypes as C
import json
import math
import os
import re
import zlib

import pytest
import torch

import grouped_oracle as go
import test_gpu_conv_forms as cf
from test_gpu_conv_forms import GUARD, TAU, U, _bound_check, _desc, _guard_ok, _out, _planes      # noqa: F401  (the bound's constants stay that file's)

# (b) on banks with fewer than 32 contracted channels per group.  Measured e(bf16x3) / e(f32), both against fp64 (profiles/grouped_forms_report.json, "ratios"):
# 1.119 at worst (Cg = 4, one accumulator; 1.080 at Kg = 4 on the transposed bank, 0.81 at Cg = 24, 0.35-0.43 with two accumulators) x 1.15, rounded up to two
# decimals.  Inputs are seeded: the margin covers a later reordering of the accumulation only.
# The depthwise forward (Cg = 1, one accumulator) measures 2.035 and carries NO bar (ratio_bar=False; rule (a) holds it at 0.31 of its bound): per tap and output
# ONE product is nonzero, fp32 MFMA (v_mfma_f32_32x32x2_f32: an exact zero adds without rounding) rounds its accumulator once for it, splitbf::mma6 six times -
# every one of the six piece-product instructions rounds the running accumulator - so the rounding count alone allows sqrt(6) = 2.45; the same count gives
# sqrt(6 / 4) = 1.22 at Cg = 4, where 1.12 is measured.  With two accumulators (mma6x2) the five small terms round a second, small accumulator: 0.35.
SPARSE_BANK_BAR = 1.29
DENSE_BAR = 1.05                                      # tests/test_gpu_split.py's bar
WORST = {}                                            # family -> worst |err| / bound (SSV_GROUPED_REPORT)
RATIOS = {}                                           # case id -> (e(bf16x3) / e(f32), the bar it is held to)
TAU_FAMILY = {"gfwd": "fwd", "gdgrad_s1": "dgrad", "gdgrad": "dgrad", "gwgrad": "wgrad"}
PRODUCT = {"gfwd": 0, "gdgrad_s1": 0, "gdgrad": 1, "gwgrad": 2}


class Case:
    def __init__(self, entry, branches, form, geom, **opt):
        self.entry, self.branches, self.form, self.geom, self.opt = entry, tuple(branches.split()), form, geom, opt
        n, h, w, c, k, r, s, pad, g = geom
        self.id = f"{entry}-{'+'.join(self.branches)}-{form}-N{n}H{h}W{w}C{c}K{k}R{r}s{s}p{pad}g{g}" + "".join(f"-{a}{b}" for a, b in sorted(opt.items()) if b not in (None, False))

    @property
    def contracted_per_group(self):
        n, h, w, c, k, r, s, pad, g = self.geom
        return (k if self.entry in ("gdgrad_s1", "gdgrad") else c) // g

    @property
    def sparse(self):
        """(b): a 32-channel k-tile of this bank holds foreign zeros between a column's own channels."""
        return self.entry in ("gfwd", "gdgrad_s1") and self.contracted_per_group % 32 != 0


# geom = (N, H, W, C, K, R(=S), stride, pad, groups)
CASES = [
    # ---- ssv_conv2d_fwd_grouped ------------------------------------------------------------------------------------------------------------
    Case("gfwd", "gfwd.span_bk32", "sp1", (2, 7, 7, 128, 128, 3, 1, 1, 32), bias=True, addend=True),
    Case("gfwd", "gfwd.span_bk32", "sp2", (1, 7, 7, 256, 256, 3, 2, 1, 32)),
    Case("gfwd", "gfwd.spans_differ", "sp1", (2, 5, 5, 128, 256, 3, 1, 1, 32), addend=True),
    Case("gfwd", "gfwd.spans_differ", "sp2", (2, 5, 5, 256, 128, 3, 1, 1, 32)),
    Case("gfwd", "gfwd.straddle", "sp2", (2, 6, 6, 192, 192, 3, 1, 1, 2), bias=True),
    Case("gfwd", "gfwd.k_ragged", "sp1", (2, 6, 6, 96, 132, 3, 1, 1, 3), bias=True, addend=True),
    Case("gfwd", "gfwd.span_rounded", "sp1", (2, 6, 6, 96, 96, 3, 1, 1, 4)),
    Case("gfwd", "gfwd.span_bk16", "f32", (2, 6, 6, 48, 96, 3, 1, 1, 3), addend=True),
    Case("gfwd", "gfwd.1x1", "sp1", (3, 7, 7, 128, 128, 1, 1, 0, 4)),
    Case("gfwd", "gfwd.taps5", "sp2", (2, 9, 9, 64, 128, 5, 2, 2, 2), bias=True, addend=True),
    Case("gfwd", "gfwd.depthwise", "sp1", (2, 6, 6, 128, 128, 3, 1, 1, 128), ratio_bar=False),
    Case("gfwd", "gfwd.dense_scalar", "f32", (2, 6, 6, 24, 24, 3, 1, 1, 3), bias=True),
    Case("gfwd", "gfwd.dense_c4", "f32", (2, 6, 6, 4, 64, 3, 1, 1, 2)),
    Case("gfwd", "gfwd.groups1", "sp1", (2, 6, 6, 64, 132, 3, 1, 1, 1), addend=True),
    # ---- stride-1 data gradient: ops.conv2d_dgrad(groups=g) ----------------------------------------------------------------------------------
    Case("gdgrad_s1", "gdgrad.s1_as_fwd", "sp2", (2, 5, 5, 128, 256, 3, 1, 1, 32), addend=True),
    Case("gdgrad_s1", "gdgrad.s1_as_fwd", "sp1", (2, 5, 5, 256, 128, 3, 1, 1, 32), addend=True),
    Case("gdgrad_s1", "gdgrad.s1_as_fwd", "sp2", (2, 6, 6, 192, 192, 3, 1, 1, 2), addend=True),
    # ---- ssv_conv2d_dgrad_grouped ------------------------------------------------------------------------------------------------------------
    Case("gdgrad", "gdgrad.bk32", "f32", (2, 9, 9, 128, 128, 3, 2, 1, 32), addend=True),
    Case("gdgrad", "gdgrad.bk16", "f32", (2, 9, 9, 96, 48, 3, 2, 1, 3)),
    Case("gdgrad", "gdgrad.no_tap_classes", "f32", (2, 7, 7, 128, 256, 1, 2, 0, 4), addend=True),
    Case("gdgrad", "gdgrad.no_tap_classes", "f32", (2, 7, 7, 128, 256, 1, 2, 0, 4)),
    Case("gdgrad", "gdgrad.stride1_entry", "f32", (2, 6, 6, 128, 64, 3, 1, 1, 16), addend=True),
    Case("gdgrad", "gdgrad.stride3", "f32", (1, 10, 10, 256, 128, 3, 3, 1, 32)),
    Case("gdgrad", "gdgrad.c_ragged", "f32", (2, 7, 7, 132, 48, 3, 2, 1, 3), addend=True),
    # ---- ssv_conv2d_wgrad_grouped ------------------------------------------------------------------------------------------------------------
    Case("gwgrad", "gwgrad.bd_s1", "sp1", (2, 7, 7, 128, 128, 3, 1, 1, 32)),
    Case("gwgrad", "gwgrad.bd_generic", "sp1", (2, 7, 7, 256, 256, 3, 2, 1, 32), accumulate=True),
    Case("gwgrad", "gwgrad.bd_lin", "sp1", (3, 5, 5, 128, 192, 1, 1, 0, 4)),
    Case("gwgrad", "gwgrad.bd_spans_differ", "sp1", (2, 5, 5, 128, 256, 3, 1, 1, 32), accumulate=True),
    Case("gwgrad", "gwgrad.dense_tiles_skip", "sp1", (3, 5, 5, 160, 160, 1, 1, 0, 5)),
    Case("gwgrad", "gwgrad.dense_tiles_noskip", "sp1", (2, 6, 6, 96, 96, 3, 1, 1, 3), accumulate=True),
    Case("gwgrad", "gwgrad.gbk", "f32", (2, 6, 6, 6, 12, 3, 1, 1, 3)),
    Case("gwgrad", "gwgrad.nsplit_ragged gwgrad.accumulate", "sp1", (3, 14, 14, 128, 128, 3, 1, 1, 32), accumulate=True),
    Case("gwgrad", "gwgrad.nsplit_ragged", "sp1", (3, 14, 14, 128, 128, 3, 1, 1, 32)),
    Case("gwgrad", "gwgrad.depthwise", "sp1", (2, 6, 6, 128, 128, 3, 1, 1, 128)),
]
BY_ID = {c.id: c for c in CASES}

# (case, poisoned groups): each pair of groups leaves a non-empty clean set and a non-empty complement, once from the spans' upper and once from their lower edge
POISON = [
    ("gfwd-gfwd.span_bk32-sp1-N2H7W7C128K128R3s1p1g32-addendTrue-biasTrue", (0, 31)),
    ("gfwd-gfwd.k_ragged-sp1-N2H6W6C96K132R3s1p1g3-addendTrue-biasTrue", (0, 2)),
    ("gdgrad_s1-gdgrad.s1_as_fwd-sp2-N2H5W5C128K256R3s1p1g32-addendTrue", (0, 31)),
    ("gdgrad-gdgrad.bk32-f32-N2H9W9C128K128R3s2p1g32-addendTrue", (0, 31)),
]


def documented_branches():
    """{(label, form)} from the module docstring's branch list."""
    out = set()
    for line in __doc__.splitlines():
        m = re.match(r"^  (g[a-z]+\.[a-z0-9_]+)\s+((?:(?:f32|sp1|sp2)\s+)+)(?:conv_mfma\.hip:[A-Za-z_]\w*|ops\.py)", line)
        if m:
            out |= {(m.group(1), f) for f in m.group(2).split()}
    return out


def covered_branches():
    out = set()
    for c in CASES:
        for b in c.branches:
            out |= {(b, "f32"), (b, c.form)}
    return out


# ============================================================================================================================ inputs and fp64 references (CPU)
_REF = {}


def reference(case):
    """The seeded fp32 operands of a case (CPU) and its fp64 reference: dict with x, wg (the GROUPED filter [K][R][S][C/g]), bank, dy, bias, addend, prior and
    ref / amag (weight gradients: [K][R][S][C/g], the diagonal blocks).  Computed once per case and shared, never written to."""
    hit = _REF.get(case.id)
    if hit is not None:
        return hit
    n, h, w, c, k, r, s, pad, g = case.geom
    ho, wo = go.out_hw(case.geom)
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    rnd = lambda *shape, scale=1.0: torch.randn(*shape, generator=gen) * scale      # noqa: E731
    cg, kg = c // g, k // g
    o = case.opt
    t = {"x": rnd(n, h, w, c), "dy": rnd(n, ho, wo, k), "bias": None, "addend": None, "prior": None}
    fan = cg if case.entry in ("gfwd", "gwgrad") else kg
    t["wg"] = rnd(k, r, r, cg, scale=(1.0 / (r * r * fan)) ** 0.5)
    t["bank"] = go.expand_bank(t["wg"], g)
    x64, dy64, wg64 = t["x"].double(), t["dy"].double(), t["wg"].double()
    if case.entry == "gfwd":
        ref, amag = go.conv64(x64, wg64, s, pad, g), go.conv64(x64.abs(), wg64.abs(), s, pad, g)
        if o.get("bias"):
            t["bias"] = rnd(k)
            ref, amag = ref + t["bias"].double(), amag + t["bias"].double().abs()
        if o.get("addend"):
            t["addend"] = rnd(n, ho, wo, k)
    elif case.entry in ("gdgrad_s1", "gdgrad"):
        ref, amag = go.dgrad64(dy64, wg64, (n, h, w, c), s, pad, g), go.dgrad64(dy64.abs(), wg64.abs(), (n, h, w, c), s, pad, g)
        if o.get("addend"):
            t["addend"] = rnd(n, h, w, c)
    else:
        ref, amag = go.wgrad64(x64, dy64, (k, r, r, cg), s, pad, g), go.wgrad64(x64.abs(), dy64.abs(), (k, r, r, cg), s, pad, g)
        if o.get("accumulate"):
            t["prior"] = rnd(k, r, r, c)
            pd = t["prior"].double()[go.diagonal_mask(case.geom)].view(k, r, r, cg)
            ref, amag = ref + pd, amag + pd.abs()
    if t["addend"] is not None:
        ref, amag = ref + t["addend"].double(), amag + t["addend"].double().abs()
    t["ref"], t["amag"] = ref, amag
    _REF[case.id] = t
    return t


# ============================================================================================================================ GPU
def _lib():
    from ssv_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    L = _lib()
    L.load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_GROUPED_REPORT")
    if path:
        rep = {"ssv_source_sha16": L.source_sha16(), "worst_err_over_bound": WORST, "SPARSE_BANK_BAR": SPARSE_BANK_BAR, "DENSE_BAR": DENSE_BAR,
               "ratios": {i: {"bf16x3_over_f32": r, "bar": bar} for i, (r, bar) in RATIOS.items()}}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)


def _bound(got, ref, amag, family, what):
    """(a) by test_gpu_conv_forms._bound_check on the CPU in fp64, the worst |err| / bound kept per family of THIS file (that file's own tally is left as it was)."""
    fam = TAU_FAMILY[family]
    saved = cf.WORST.pop(fam, None)
    try:
        _bound_check(got.cpu(), ref, amag, fam, what)
    finally:
        seen = cf.WORST.pop(fam, 0.0)
        WORST[family] = max(WORST.get(family, 0.0), seen)
        if saved is not None:
            cf.WORST[fam] = saved


def _rel(got, ref):
    return float((got.cpu().double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _to(t, dev):
    return None if t is None else t.to(dev)


def _ohwi_view(bank):
    """the bank [K][R][S][C] as the channels_last [K, C, R, S] tensor ops takes"""
    return bank.permute(0, 3, 1, 2)


def _launch(case, arith, dev, x=None, dy=None, planes_on_dgrad=False):
    """One launch of a case in one arithmetic: dict(out, buf, dense, desc, extra...).  ``x`` / ``dy``: a replacement for the contracted operand (the poison test)."""
    from ssv_amd import ops
    L = _lib()
    P, lib = L.ptr, L.load()
    n, h, w, c, k, r, s, pad, g = case.geom
    ho, wo = go.out_hw(case.geom)
    t = reference(case)
    geom8 = case.geom[:8]
    keep, res = [], {}
    bank = t["bank"].to(dev)
    xd = _to(t["x"], dev) if x is None else x
    dyd = _to(t["dy"], dev) if dy is None else dy
    add, bias = _to(t["addend"], dev), _to(t["bias"], dev)
    with ops.arithmetic(arith):
        stream = L.stream()
        if case.entry == "gfwd":
            d = _desc(geom8, arith, bank, keep)
            buf, y = _out((n, ho, wo, k), dev)
            L.call("ssv_conv2d_fwd_grouped", C.byref(d), g, P(xd), P(bank), P(bias), P(add), P(y), stream)
            dense = torch.empty_like(y)
            L.call("ssv_conv2d_fwd", C.byref(d), P(xd), P(bank), P(bias), P(add), P(dense), stream)
            res.update(out=y, buf=buf, dense=dense, desc=d)
        elif case.entry == "gdgrad_s1":
            wc = _ohwi_view(bank)
            buf, dx = _out((n, h, w, c), dev)
            got = ops.conv2d_dgrad(dyd, wc, (n, h, w, c), 1, pad, addend=add, out=dx, groups=g)
            assert got.data_ptr() == dx.data_ptr()
            dense = ops.conv2d_dgrad(dyd, wc, (n, h, w, c), 1, pad, addend=add)
            wt = ops._transposed_filter(wc, (k, c, r, r))
            res.update(out=dx, buf=buf, dense=dense, desc=_desc((n, ho, wo, k, c, r, 1, r - 1 - pad), arith, wt, keep))
        elif case.entry == "gdgrad":
            d = _desc(geom8, arith)                                   # as ops builds it for a bank: no planes
            buf, dx = _out((n, h, w, c), dev)
            L.call("ssv_conv2d_dgrad_grouped", C.byref(d), g, P(dyd), P(bank), P(add), P(dx), stream)
            res.update(out=dx, buf=buf, desc=d, dense=None)
            if arith == "f32" or c < 128:                             # (f): both run the 256 x 64 fp32-MFMA kernel
                res["dense"] = torch.empty_like(dx)
                L.call("ssv_conv2d_dgrad", C.byref(d), P(dyd), P(bank), P(add), P(res["dense"]), stream)
            if planes_on_dgrad and arith == "bf16x3":                 # (b): planes on the descriptor change nothing
                dp = _desc(geom8, arith, bank, keep)
                assert dp.w_planes and dp.arithmetic == L.ARITH_BF16X3
                bufp, dxp = _out((n, h, w, c), dev)
                L.call("ssv_conv2d_dgrad_grouped", C.byref(dp), g, P(dyd), P(bank), P(add), P(dxp), stream)
                res.update(with_planes=dxp, buf_planes=bufp)
        else:
            d = _desc(geom8, arith)
            plan = go.WgradPlan(case.geom)
            wsb = int(lib.ssv_conv2d_wgrad_grouped_workspace_bytes(C.byref(d), g))
            assert wsb == plan.workspace_bytes, f"plan_wgrad changed: update grouped_oracle.WgradPlan ({wsb} != {plan.workspace_bytes})"
            wsbuf = torch.full((wsb // 4 + GUARD,), float("nan"), device=dev)
            acc = bool(case.opt.get("accumulate"))
            buf, dw = _out((k, r, r, c), dev, _to(t["prior"], dev))
            L.call("ssv_conv2d_wgrad_grouped", C.byref(d), g, P(xd), P(dyd), P(dw), int(acc), P(wsbuf), wsb, stream)
            res.update(out=dw, buf=buf, desc=d, ws=wsbuf, plan=plan, dense=None)
        torch.cuda.synchronize()
    res["keep"] = keep
    return res


def _check_wgrad_bank(case, res, what):
    """(e) for a bank-layout weight gradient and "skipped tiles": returns the diagonal blocks [K][R][S][C/g]."""
    n, h, w, c, k, r, s, pad, g = case.geom
    dw, buf, wsbuf, plan = res["out"].cpu(), res["buf"].cpu(), res["ws"].cpu(), res["plan"]
    nw, nws = k * r * r * c, plan.workspace_bytes // 4
    assert torch.isnan(buf[nw:]).all(), f"{what}: wrote past the end of dwd"
    assert torch.isnan(wsbuf[nws:]).all(), f"{what}: wrote past the end of the workspace"
    skipped, diag = go.skipped_mask(case.geom), go.diagonal_mask(case.geom)
    assert not (skipped & diag).any(), "the restated skip rule skips a diagonal entry"
    assert torch.isfinite(dw[diag]).all(), f"{what}: non-finite entries in the diagonal blocks"
    assert torch.isnan(dw[skipped]).all(), f"{what}: {int((~torch.isnan(dw[skipped])).sum())} entries of skipped tiles were written (the skip branch was not taken)"
    assert torch.isfinite(dw[~skipped]).all(), f"{what}: non-finite entries in worked tiles"
    slabs = wsbuf[:nws].view(plan.nsplit, k, r, r, c)
    for i in range(plan.nsplit):
        assert torch.isnan(slabs[i][skipped]).all(), f"{what}: slab {i}: entries of skipped tiles were written"
        assert torch.isfinite(slabs[i][~skipped]).all(), f"{what}: slab {i}: worked tiles left unwritten or non-finite"
    return dw[diag].view(k, r, r, c // g)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_grouped_launch_form_against_fp64_in_both_arithmetics(dev, case):
    L = _lib()
    lib = L.load()
    t = reference(case)
    got = {}
    for arith in ("f32", "bf16x3"):
        res = _launch(case, arith, dev, planes_on_dgrad=True)
        what = f"{case.id} [{arith}]"
        # (c) the launched arithmetic
        want = L.ARITH_BF16X3 if (arith == "bf16x3" and case.form != "f32") else L.ARITH_F32_MFMA
        assert lib.ssv_conv_arithmetic(C.byref(res["desc"]), PRODUCT[case.entry]) == want, f"{what}: ssv_conv_arithmetic is not {case.form}"
        # (e) guards, (a) the bound
        if case.entry == "gwgrad":
            out = _check_wgrad_bank(case, res, what)
        else:
            _guard_ok(res["buf"], what)
            out = res["out"]
        print(f"{what}: rel l2 {_rel(out, t['ref']):.3e}")
        _bound(out, t["ref"], t["amag"], case.entry, what)
        # (f) the dense entry point on the same bank
        if res["dense"] is not None:
            assert torch.equal(res["out"], res["dense"]), f"{what}: not bit-identical to the dense entry point on the same bank"
        if case.entry in ("gfwd", "gdgrad_s1"):
            assert res["dense"] is not None
        if "with_planes" in res:
            _guard_ok(res["buf_planes"], what + " (planes attached)")
            assert torch.equal(res["out"], res["with_planes"]), f"{what}: planes on the descriptor changed the grouped strided data gradient"
        got[arith] = out.cpu()
        del res
    # (b) the two arithmetics
    if case.form == "f32":
        assert torch.equal(got["f32"], got["bf16x3"]), f"{case.id}: no bf16-piece form, yet the two arithmetics differ"
    else:
        e32, esp = _rel(got["f32"], t["ref"]), _rel(got["bf16x3"], t["ref"])
        ratio = esp / max(e32, 1e-300)
        RATIOS[case.id] = (ratio, "none: rule (a) only" if case.opt.get("ratio_bar") is False else ("SPARSE_BANK_BAR" if case.sparse else "DENSE_BAR"))
        print(f"{case.id}: e(bf16x3) / e(f32) = {esp:.3e} / {e32:.3e} = {ratio:.3f} ({'sparse' if case.sparse else 'dense'} bank bar)")
        bar = SPARSE_BANK_BAR if case.sparse else DENSE_BAR
        if case.opt.get("ratio_bar") is False:
            assert case.sparse and case.contracted_per_group == 1, "only the depthwise forward goes without a ratio bar (see SPARSE_BANK_BAR)"
            return
        assert esp <= bar * e32 + 1e-9, f"{case.id}: bf16x3 {esp:.3e} vs fp32 MFMA {e32:.3e} against fp64 (ratio {ratio:.3f}, bar {bar}x)"


@pytest.mark.gpu
@pytest.mark.parametrize("cid,group", [(cid, grp) for cid, groups in POISON for grp in groups], ids=lambda v: str(v))
def test_poisoned_group_stays_outside_the_span(dev, cid, group):
    """One group's contracted channels (x for the forward, dy for the data gradients) are NaN - data, every index stays in range.  Columns whose tile's span
    excludes them are finite and inside (a); the dense entry point, which contracts over everything, is non-finite there: the poison was live."""
    case = BY_ID[cid]
    t = reference(case)
    n, h, w, c, k, r, s, pad, g = case.geom
    clean = go.clean_columns(case.entry, case.geom, group)
    assert clean.any() and not clean.all()
    key = "x" if case.entry == "gfwd" else "dy"
    per = case.contracted_per_group
    bad = t[key].clone()
    bad[..., group * per:(group + 1) * per] = float("nan")
    for arith in ("f32", "bf16x3"):
        what = f"{case.id} group {group} poisoned [{arith}]"
        res = _launch(case, arith, dev, **{key: bad.to(dev)})
        out = res["out"].cpu()
        assert torch.isnan(res["buf"][out.numel():]).all(), f"{what}: wrote past the end of its output"
        assert torch.isfinite(out[..., clean]).all(), f"{what}: a column outside the span saw the poisoned channels"
        _bound(out[..., clean], t["ref"][..., clean], t["amag"][..., clean], case.entry, what)
        if res["dense"] is None:                                      # bf16x3 on C >= 128: the dense strided kernel is another launch form, equally dense
            L = _lib()
            d = res["desc"]
            res["dense"] = torch.empty_like(res["out"])
            operands = (bad.to(dev), t["bank"].to(dev), _to(t["addend"], dev))          # held until the launch has run
            L.call("ssv_conv2d_dgrad", C.byref(d), *(L.ptr(v) for v in operands), L.ptr(res["dense"]), L.stream())
            torch.cuda.synchronize()
            del operands
        assert not torch.isfinite(res["dense"].cpu()[..., clean]).any(), f"{what}: the dense entry point stayed finite - the poison was not live"


@pytest.mark.gpu
def test_refusals(dev):
    """Every refused call returns its error before anything is launched: outputs (n floats of prefill, then GUARD floats of NaN) stay bit for bit."""
    L = _lib()
    P, lib = L.ptr, L.load()
    ERR_INVALID, ERR_WORKSPACE = -1, -2
    stream = L.stream()

    def desc(n, h, w, c, k, r, s, pad):
        return _desc((n, h, w, c, k, r, s, pad), "f32")

    def prefilled(nfloats):
        buf = torch.full((nfloats + GUARD,), float("nan"), device=dev)
        buf[:nfloats] = 7.25
        return buf, buf.clone()

    def untouched(pair, what):
        torch.cuda.synchronize()
        assert torch.equal(pair[0].view(torch.int32), pair[1].view(torch.int32)), f"{what}: a refused call wrote to its output"

    n, h, w, c, k = 2, 6, 6, 96, 96
    d = desc(n, h, w, c, k, 3, 1, 1)
    x, dy, bank = torch.randn(n, h, w, c, device=dev), torch.randn(n, h, w, k, device=dev), torch.randn(k, 3, 3, c, device=dev)
    y, dx, dw = prefilled(n * h * w * k), prefilled(n * h * w * c), prefilled(k * 9 * c)
    wsb = int(lib.ssv_conv2d_wgrad_grouped_workspace_bytes(C.byref(d), 3))
    assert wsb > 0
    ws = prefilled(wsb // 4)
    outs = ((y, "y"), (dx, "dx"), (dw, "dwd"), (ws, "workspace"))

    def fwd(dd, g, xp, wp, yp):
        return lib.ssv_conv2d_fwd_grouped(C.byref(dd), g, xp, wp, None, None, yp, stream)

    def dgrad(dd, g, dyp, wp, dxp):
        return lib.ssv_conv2d_dgrad_grouped(C.byref(dd), g, dyp, wp, None, dxp, stream)

    def wgrad(dd, g, xp, dyp, dwp, wsp, nbytes):
        return lib.ssv_conv2d_wgrad_grouped(C.byref(dd), g, xp, dyp, dwp, 0, wsp, nbytes, stream)

    X, DY, B, Y, DX, DW, WS = P(x), P(dy), P(bank), P(y[0]), P(dx[0]), P(dw[0]), P(ws[0])
    calls = []
    for g in (5, 0, -1):                                 # 5 divides neither 96 nor 96
        calls += [(f"fwd groups={g}", lambda g=g: fwd(d, g, X, B, Y)), (f"dgrad groups={g}", lambda g=g: dgrad(d, g, DY, B, DX)),
                  (f"wgrad groups={g}", lambda g=g: wgrad(d, g, X, DY, DW, WS, wsb))]
    d_ck = desc(n, h, w, 96, 64, 3, 1, 1)                # groups that divide C but not K, and the reverse (buffers above are large enough for either)
    calls += [("fwd groups | C only", lambda: fwd(d_ck, 3, X, B, Y)), ("dgrad groups | K only", lambda: dgrad(desc(n, h, w, 64, 96, 3, 1, 1), 3, DY, B, DX)),
              ("wgrad groups | C only", lambda: wgrad(d_ck, 3, X, DY, DW, WS, wsb))]
    calls += [("fwd null x", lambda: fwd(d, 3, None, B, Y)), ("fwd null wd", lambda: fwd(d, 3, X, None, Y)), ("fwd null y", lambda: fwd(d, 3, X, B, None)),
              ("fwd misaligned x", lambda: fwd(d, 3, X + 4, B, Y)), ("fwd misaligned wd", lambda: fwd(d, 3, X, B + 4, Y)), ("fwd misaligned y", lambda: fwd(d, 3, X, B, Y + 4)),
              ("dgrad null dy", lambda: dgrad(d, 3, None, B, DX)), ("dgrad null wd", lambda: dgrad(d, 3, DY, None, DX)), ("dgrad null dx", lambda: dgrad(d, 3, DY, B, None)),
              ("dgrad misaligned dy", lambda: dgrad(d, 3, DY + 4, B, DX)), ("dgrad misaligned dx", lambda: dgrad(d, 3, DY, B, DX + 4)),
              ("wgrad null x", lambda: wgrad(d, 3, None, DY, DW, WS, wsb)), ("wgrad null dy", lambda: wgrad(d, 3, X, None, DW, WS, wsb)),
              ("wgrad null dwd", lambda: wgrad(d, 3, X, DY, None, WS, wsb)), ("wgrad null workspace", lambda: wgrad(d, 3, X, DY, DW, None, wsb)),
              ("wgrad misaligned dwd", lambda: wgrad(d, 3, X, DY, DW + 4, WS, wsb)), ("wgrad misaligned workspace", lambda: wgrad(d, 3, X, DY, DW, WS + 4, wsb)),
              ("null descriptor fwd", lambda: lib.ssv_conv2d_fwd_grouped(None, 3, X, B, None, None, Y, stream)),
              ("dgrad K % 16 != 0", lambda: dgrad(desc(n, h, w, 96, 24, 3, 1, 1), 3, DY, B, DX)),
              ("dgrad C % 4 != 0", lambda: dgrad(desc(n, h, w, 6, 32, 3, 1, 1), 2, DY, B, DX)),
              ("wgrad K % 4 != 0", lambda: wgrad(desc(n, h, w, 96, 6, 3, 1, 1), 3, X, DY, DW, WS, wsb))]
    for name, fn in calls:
        assert fn() == ERR_INVALID, f"{name}: not refused with SSV_ERR_INVALID"
        assert lib.ssv_last_error(), name
        for pair, what in outs:
            untouched(pair, f"{name}: {what}")
    # a workspace one byte short
    assert wgrad(d, 3, X, DY, DW, WS, wsb - 1) == ERR_WORKSPACE
    msg = lib.ssv_last_error().decode()
    assert str(wsb) in msg and str(wsb - 1) in msg, msg
    for pair, what in outs:
        untouched(pair, f"short workspace: {what}")
    # the size query's own refusals
    q = lib.ssv_conv2d_wgrad_grouped_workspace_bytes
    assert q(None, 3) == 0 and q(C.byref(d), 0) == 0 and q(C.byref(d), -1) == 0 and q(C.byref(d), 5) == 0 and q(C.byref(d_ck), 3) == 0
    # and the accepted call still runs afterwards
    assert wgrad(d, 3, X, DY, DW, WS, wsb) == 0
    torch.cuda.synchronize()
    assert torch.isnan(dw[0][k * 9 * c:]).all() and torch.isnan(ws[0][wsb // 4:]).all()
