"""Every launch form of the conv-family entry points (csrc/conv_mfma.hip) against an fp64 evaluation, in BOTH arithmetics.

Each case of CASES names the entry point it calls (straight through the C ABI, or through ops.* where ops is the only caller of a route), the
branch of the launch selection it targets and the form that branch takes under SSV_ARITH_BF16X3: "sp1" (one accumulator, R*S*C <= SP_DUAL_FROM =
1152), "sp2" (two accumulators beyond) or "f32" (no bf16-piece kernel: the bf16x3 request runs on fp32 MFMA).  Every case runs once under
ops.arithmetic("f32") and once under ops.arithmetic("bf16x3"), and each run is held to:

  (a) element-wise: |got - ref| <= TAU * 2^-24 * A + floor, where A is the same fp64 operation on the absolute values of the operands (fp32
      accumulation of n products errs by a small multiple of 2^-24 * sum |a b|; TAU is fixed once per family, never per case);
  (b) on cases with a bf16x3 form: the bf16x3 relative l2 error against fp64 <= 1.05 x the fp32-MFMA one + 1e-9 (tests/test_gpu_split.py's bar;
      1.15 x for one-accumulator forwards of a ReLU formed on load, see SPARSE_SP1_BAR);
      on cases without one: the two runs are the same launch and bit-identical;
  (c) ssv_conv_arithmetic(desc, product) reports the case's form;
  (d) statistics / gate partials per 64-row group against fp64 sums of the rows the kernel wrote; the group count is the library's
      *_groups answer for that descriptor, and groups past the rows are zero;
  (e) every output is a view into a NaN-prefilled buffer: nothing of the output is left NaN, nothing of the guard behind it is written;
  (f) the bitwise identities the code states: fused forward variants == the plain forward on the materialised operand, the closing-activation
      forward == ssv_bn_apply + ssv_conv2d_fwd_stats, gated outputs == the masked plain output.

Branches (label, forms, the function of conv_mfma.hip that selects it) - test_case_table_covers_every_documented_branch keeps CASES honest:

  fwd.wide                 f32 sp1 sp2   conv_mfma.hip:fwd_tile  ssv_conv2d_fwd, float4 path, 128x128 tile (K >= 128)
  fwd.narrow               f32 sp1 sp2   conv_mfma.hip:fwd_tile  ssv_conv2d_fwd, float4 path, 256x64 (f32) / 128x64 (bf16x3) tile
  fwd.bk16                 f32           conv_mfma.hip:launch_fwd  ssv_conv2d_fwd, C % 16 == 0 but not % 32
  fwd.generic              f32           conv_mfma.hip:launch_fwd  ssv_conv2d_fwd, C % 16 != 0 (scalar gather)
  fwd.k_unaligned          f32           conv_mfma.hip:launch_fwd  ssv_conv2d_fwd, K % 4 != 0 (scalar epilogue)
  fwd.stats                f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_stats
  fwd.xf                   f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_bnrelu_in_stats, fused input only
  fwd.xf_stats             f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_bnrelu_in_stats, fused input + statistics
  fwd.gate_affine          f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_gated, scale / shift gate
  fwd.gate_mask            f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_gated, byte-mask gate
  fwd.gate_x2              f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_gated, byte mask + second target x2
  fwd.gate_s2add           f32 sp1 sp2   conv_mfma.hip:launch_fwd  ssv_conv2d_fwd_gated_s2add (mask, mask + x2)
  fwd.dyin                 f32 sp1 sp2   conv_mfma.hip:fwd_dyin_impl  ssv_conv2d_fwd_dyin, no gate
  fwd.dyin_gate            f32 sp1 sp2   conv_mfma.hip:fwd_dyin_impl  ssv_conv2d_fwd_dyin with affine / mask / x2 gates
  fwd.dyin_s2add           f32 sp1 sp2   conv_mfma.hip:fwd_dyin_impl  ssv_conv2d_fwd_dyin_s2add
  fwd.sumin                f32 sp1 sp2   conv_mfma.hip:ssv_conv2d_fwd_sumin_stats  ssv_conv2d_fwd_sumin_stats (+- rscale / rshift, +- mask_out)
  lin.gelu                 f32 sp1 sp2   conv_mfma.hip:ssv_linear_gelu_fwd  ssv_linear_gelu_fwd (h kept / act only)
  lin.gelu_dact            f32 sp1 sp2   conv_mfma.hip:ssv_linear_gelu_fwd_dact  ssv_linear_gelu_fwd_dact
  lin.mulgrad              f32 sp1 sp2   conv_mfma.hip:ssv_linear_fwd_mulgrad  ssv_linear_fwd_mulgrad
  lin.gelugrad             f32 sp1 sp2   conv_mfma.hip:ssv_linear_fwd_gelugrad  ssv_linear_fwd_gelugrad
  dgrad.gelu               f32           conv_mfma.hip:ssv_conv2d_dgrad_gelu  ssv_conv2d_dgrad_gelu (strided kernel, fp32 only)
  dgrad.s1_as_fwd          f32 sp1 sp2   ops.py conv2d_dgrad  stride 1: forward kernel on the transposed filter (conv_mfma.hip:fwd_tile)
  dgrad.wide_bk32          f32 sp1       conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad, C >= 128, K % 32 == 0
  dgrad.wide_bk16          f32           conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad, C >= 128, K % 16 only
  dgrad.narrow_bk32        f32           conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad, C < 128, K % 32 == 0
  dgrad.narrow_bk16        f32           conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad, C < 128, K % 16 only
  dgrad.gate_wide          f32 sp1       conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad_gated, C >= 128 (affine, mask)
  dgrad.gate_narrow        f32           conv_mfma.hip:dgrad_tile  ssv_conv2d_dgrad_gated, C < 128 (affine, mask)
  wgrad.lin                f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad, LIN gather (1x1 / s1 / p0)
  wgrad.s1                 f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad, S1 gather (stride 1, 32 / Wo + 1 <= Ho)
  wgrad.generic            f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad, generic gather (strided, tiny maps)
  wgrad.gbk                f32           conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad, C % 4 != 0
  wgrad.bm128_bn64         f32 sp1       conv_mfma.hip:plan_wgrad  128-row tile, 64-column tile (R*S*C <= 64)
  wgrad.bm64_bn64          f32 sp1       conv_mfma.hip:plan_wgrad  64-row tile, 64-column tile
  wgrad.bm128_bn128        f32 sp1       conv_mfma.hip:plan_wgrad  128 x 128 tile
  wgrad.bm64_bn128         f32 sp1       conv_mfma.hip:plan_wgrad  64 x 128 tile
  wgrad.nsplit_ragged      f32 sp1       conv_mfma.hip:wgrad_row_split  plan_wgrad: several row chunks, the last one short
  wgrad.accumulate         f32 sp1       conv_mfma.hip:wgrad_impl  dw += on a nonzero prior
  wgrad.xf                 f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad_bnrelu_in (LIN, S1, generic)
  wgrad.dyin               f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad_dyin (+- in_affine)
  wgrad.bias               f32 sp1       conv_mfma.hip:wgrad_impl  ssv_conv2d_wgrad_bias
"""
import ctypes as C
import json
import math
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TAU = {"fwd": 16.0, "dgrad": 16.0, "wgrad": 16.0, "partials": 16.0}      # fixed per family from the fp32 accumulation argument above
GUARD = 1024                                                              # floats of NaN behind every output
# (b) on a forward whose operand is a ReLU formed on load (fused input, closing activation: about half of it exact zeros) with ONE accumulator: measured
# 1.07-1.13x the fp32-MFMA error.  A zero product costs fp32 MFMA no rounding, while the bf16x3 form rounds once per instruction of 32 products whatever
# they are; both stay far inside bound (a).  Every other case keeps test_gpu_split's 1.05x.
SPARSE_SP1_BAR = 1.15
WORST = {}                                                                # family -> worst |err| / bound seen (reported by SSV_FORMS_REPORT)


class Case:
    def __init__(self, entry, branches, form, geom, **opt):
        self.entry, self.branches, self.form, self.geom, self.opt = entry, tuple(branches.split()), form, geom, opt
        n, h, w, c, k, r, s, pad = geom
        self.id = f"{entry}-{'+'.join(self.branches)}-{form}-N{n}H{h}W{w}C{c}K{k}R{r}s{s}p{pad}" + "".join(f"-{a}{b}" for a, b in sorted(opt.items()) if b not in (None, False))


# geom = (N, H, W, C, K, R(=S), stride, pad)
CASES = [
    # ---- forward family ------------------------------------------------------------------------------------------------------------------
    Case("fwd", "fwd.wide", "sp1", (2, 9, 9, 32, 132, 3, 1, 1), bias=True, addend=True),
    Case("fwd", "fwd.wide", "sp1", (1, 11, 11, 128, 128, 3, 1, 1)),                          # R*S*C = 1152: the boundary, one accumulator
    Case("fwd", "fwd.wide", "sp2", (1, 7, 7, 160, 260, 3, 1, 1), addend=True),
    Case("fwd", "fwd.wide", "sp2", (2, 5, 5, 2048, 132, 1, 1, 0), bias=True),
    Case("fwd", "fwd.narrow", "sp1", (3, 9, 9, 64, 68, 3, 2, 1), bias=True, addend=True),
    Case("fwd", "fwd.narrow", "sp1", (1, 11, 11, 128, 64, 3, 1, 1)),
    Case("fwd", "fwd.narrow", "sp2", (1, 9, 9, 160, 68, 3, 1, 1), addend=True),
    Case("fwd", "fwd.narrow", "sp2", (3, 7, 7, 2048, 64, 1, 1, 0)),
    Case("fwd", "fwd.k_unaligned", "f32", (2, 7, 7, 32, 66, 3, 1, 1), bias=True, addend=True),
    Case("fwd", "fwd.bk16", "f32", (2, 9, 9, 48, 132, 3, 1, 1), addend=True),
    Case("fwd", "fwd.bk16", "f32", (2, 9, 9, 16, 68, 3, 2, 1)),
    Case("fwd", "fwd.generic", "f32", (2, 8, 8, 20, 68, 3, 1, 1), bias=True),
    Case("fwd", "fwd.generic fwd.k_unaligned", "f32", (3, 6, 6, 12, 130, 3, 2, 1), addend=True),
    Case("stats", "fwd.stats", "sp1", (3, 9, 9, 32, 132, 3, 1, 1)),
    Case("stats", "fwd.stats", "sp1", (5, 7, 7, 64, 68, 1, 1, 0)),
    Case("stats", "fwd.stats", "sp2", (2, 7, 7, 160, 64, 3, 1, 1)),
    Case("stats", "fwd.stats", "sp2", (1, 9, 9, 160, 260, 3, 2, 1)),
    Case("xf", "fwd.xf", "sp1", (2, 9, 9, 64, 132, 3, 1, 1)),
    Case("xf", "fwd.xf_stats", "sp1", (3, 7, 7, 96, 68, 3, 1, 1), stats=True),
    Case("xf", "fwd.xf", "sp2", (2, 7, 7, 160, 68, 3, 1, 1)),
    Case("xf", "fwd.xf_stats", "sp2", (2, 7, 7, 192, 132, 3, 2, 1), stats=True),
    Case("gated", "fwd.gate_affine", "sp1", (2, 9, 9, 64, 132, 3, 1, 1), gate="affine", addend=True),
    Case("gated", "fwd.gate_affine", "sp1", (3, 7, 7, 32, 68, 3, 1, 1), gate="affine"),
    Case("gated", "fwd.gate_affine", "sp2", (2, 7, 7, 160, 68, 3, 1, 1), gate="affine", addend=True),
    Case("gated", "fwd.gate_mask", "sp1", (3, 7, 7, 256, 64, 1, 1, 0), gate="mask", addend=True),
    Case("gated", "fwd.gate_mask", "sp2", (1, 9, 9, 160, 260, 3, 1, 1), gate="mask"),
    Case("gated", "fwd.gate_x2", "sp1", (3, 7, 7, 64, 256, 1, 1, 0), gate="x2", addend=True),
    Case("gated", "fwd.gate_x2", "sp2", (2, 5, 5, 1280, 68, 1, 1, 0), gate="x2"),
    Case("s2add", "fwd.gate_s2add", "sp1", (2, 7, 7, 64, 256, 1, 1, 0), gate="mask"),
    Case("s2add", "fwd.gate_s2add", "sp1", (3, 6, 6, 128, 132, 1, 1, 0), gate="x2"),
    Case("s2add", "fwd.gate_s2add", "sp2", (2, 5, 5, 1280, 128, 1, 1, 0), gate="x2"),
    Case("dyin", "fwd.dyin", "sp1", (3, 7, 7, 256, 64, 1, 1, 0)),
    Case("dyin", "fwd.dyin", "sp2", (2, 7, 7, 2048, 132, 1, 1, 0), addend=True),
    Case("dyin", "fwd.dyin_gate", "sp1", (2, 9, 9, 128, 512, 1, 1, 0), gate="affine", addend=True),
    Case("dyin", "fwd.dyin_gate", "sp1", (3, 7, 7, 64, 68, 1, 1, 0), gate="mask"),
    Case("dyin", "fwd.dyin_gate", "sp2", (2, 5, 5, 1280, 64, 1, 1, 0), gate="x2", addend=True),
    Case("dyin_s2add", "fwd.dyin_s2add", "sp1", (2, 7, 7, 256, 128, 1, 1, 0), gate="mask"),
    Case("dyin_s2add", "fwd.dyin_s2add", "sp2", (2, 5, 5, 1280, 132, 1, 1, 0), gate="x2"),
    Case("sumin", "fwd.sumin", "sp1", (3, 9, 9, 64, 68, 1, 1, 0), raff=True, mask=True),
    Case("sumin", "fwd.sumin", "sp1", (2, 7, 7, 256, 132, 1, 1, 0)),
    Case("sumin", "fwd.sumin", "sp2", (2, 7, 7, 1280, 64, 1, 1, 0), raff=True),
    Case("sumin", "fwd.sumin", "sp2", (1, 9, 9, 2048, 256, 1, 1, 0), mask=True),
    Case("gelu", "lin.gelu", "sp1", (300, 1, 1, 256, 132, 1, 1, 0), keep_h=True),
    Case("gelu", "lin.gelu", "sp1", (200, 1, 1, 96, 256, 1, 1, 0), keep_h=False),
    Case("gelu", "lin.gelu", "sp2", (130, 1, 1, 1536, 260, 1, 1, 0), keep_h=True),
    Case("gelu", "lin.gelu", "sp2", (70, 1, 1, 1536, 128, 1, 1, 0), keep_h=False),
    Case("gelu_dact", "lin.gelu_dact", "sp1", (300, 1, 1, 256, 132, 1, 1, 0)),
    Case("gelu_dact", "lin.gelu_dact", "sp2", (130, 1, 1, 1536, 260, 1, 1, 0)),
    Case("mulgrad", "lin.mulgrad", "sp1", (300, 1, 1, 256, 132, 1, 1, 0), addend=True),
    Case("mulgrad", "lin.mulgrad", "sp2", (130, 1, 1, 1536, 260, 1, 1, 0)),
    Case("gelugrad", "lin.gelugrad", "sp1", (300, 1, 1, 256, 132, 1, 1, 0)),
    Case("gelugrad", "lin.gelugrad", "sp2", (130, 1, 1, 1536, 260, 1, 1, 0), addend=True),
    Case("dgrad_gelu", "dgrad.gelu", "f32", (300, 1, 1, 132, 256, 1, 1, 0), addend=True),
    # ---- data gradient -------------------------------------------------------------------------------------------------------------------
    Case("dgrad_s1", "dgrad.s1_as_fwd", "sp1", (2, 9, 9, 64, 128, 3, 1, 1), addend=True),
    Case("dgrad_s1", "dgrad.s1_as_fwd", "sp2", (2, 7, 7, 132, 160, 3, 1, 1), addend=True),
    Case("dgrad", "dgrad.wide_bk32", "sp1", (2, 10, 10, 128, 64, 3, 2, 1), addend=True),
    Case("dgrad", "dgrad.wide_bk32", "sp1", (3, 9, 9, 136, 96, 3, 2, 1), addend="alias"),
    Case("dgrad", "dgrad.wide_bk32", "sp1", (2, 11, 11, 256, 64, 1, 3, 0)),
    Case("dgrad", "dgrad.wide_bk32", "sp1", (1, 13, 13, 136, 32, 3, 4, 1), addend=True),
    Case("dgrad", "dgrad.wide_bk16", "f32", (2, 9, 9, 128, 48, 3, 2, 1), addend="alias"),
    Case("dgrad", "dgrad.wide_bk16", "f32", (2, 8, 8, 256, 16, 1, 2, 0)),
    Case("dgrad", "dgrad.narrow_bk32", "f32", (3, 10, 10, 64, 64, 3, 2, 1), addend=True),
    Case("dgrad", "dgrad.narrow_bk32", "f32", (2, 11, 11, 36, 96, 3, 3, 1), addend="alias"),
    Case("dgrad", "dgrad.narrow_bk16", "f32", (2, 9, 9, 32, 48, 3, 2, 1)),
    Case("dgrad", "dgrad.narrow_bk16", "f32", (2, 12, 12, 64, 16, 1, 4, 0), addend=True),
    Case("dgrad_gated", "dgrad.gate_wide", "sp1", (2, 10, 10, 128, 64, 3, 2, 1), gate="affine", addend=True),
    Case("dgrad_gated", "dgrad.gate_wide", "sp1", (2, 9, 9, 256, 96, 1, 2, 0), gate="mask"),
    Case("dgrad_gated", "dgrad.gate_wide", "sp1", (1, 11, 11, 136, 32, 3, 3, 1), gate="mask", addend=True),
    Case("dgrad_gated", "dgrad.gate_narrow", "f32", (3, 9, 9, 64, 64, 3, 2, 1), gate="affine"),
    Case("dgrad_gated", "dgrad.gate_narrow", "f32", (2, 10, 10, 32, 96, 1, 2, 0), gate="mask", addend=True),
    # ---- weight gradient -----------------------------------------------------------------------------------------------------------------
    Case("wgrad", "wgrad.lin wgrad.bm128_bn64", "sp1", (3, 7, 7, 64, 128, 1, 1, 0)),
    Case("wgrad", "wgrad.lin wgrad.bm64_bn64 wgrad.accumulate", "sp1", (2, 9, 9, 32, 68, 1, 1, 0), accumulate=True),
    Case("wgrad", "wgrad.lin wgrad.bm128_bn128 wgrad.nsplit_ragged", "sp1", (37, 14, 14, 256, 132, 1, 1, 0)),
    Case("wgrad", "wgrad.lin wgrad.bm64_bn128 wgrad.accumulate", "sp1", (4, 9, 9, 160, 64, 1, 1, 0), accumulate=True),
    Case("wgrad", "wgrad.s1 wgrad.bm128_bn128", "sp1", (2, 9, 9, 64, 128, 3, 1, 1)),
    Case("wgrad", "wgrad.s1 wgrad.bm64_bn128 wgrad.nsplit_ragged", "sp1", (21, 12, 12, 32, 64, 3, 1, 1)),
    Case("wgrad", "wgrad.generic wgrad.bm128_bn128", "sp1", (3, 9, 9, 64, 256, 3, 2, 1), accumulate=True),
    Case("wgrad", "wgrad.generic wgrad.bm64_bn128", "sp1", (5, 4, 4, 32, 64, 3, 1, 1)),
    Case("wgrad", "wgrad.generic wgrad.bm64_bn64", "sp1", (4, 7, 7, 4, 68, 3, 2, 1)),
    Case("wgrad", "wgrad.gbk", "f32", (3, 8, 8, 6, 132, 3, 1, 1)),
    Case("wgrad", "wgrad.gbk wgrad.accumulate", "f32", (2, 9, 9, 3, 64, 3, 2, 1), accumulate=True),
    Case("wgrad_xf", "wgrad.xf wgrad.lin", "sp1", (3, 7, 7, 64, 128, 1, 1, 0)),
    Case("wgrad_xf", "wgrad.xf wgrad.s1", "sp1", (2, 9, 9, 32, 64, 3, 1, 1), accumulate=True),
    Case("wgrad_xf", "wgrad.xf wgrad.generic", "sp1", (3, 9, 9, 64, 132, 3, 2, 1)),
    Case("wgrad_dyin", "wgrad.dyin wgrad.lin", "sp1", (3, 7, 7, 64, 256, 1, 1, 0)),
    Case("wgrad_dyin", "wgrad.dyin wgrad.lin wgrad.accumulate", "sp1", (2, 9, 9, 160, 64, 1, 1, 0), in_affine=True, accumulate=True),
    Case("wgrad_bias", "wgrad.bias wgrad.lin", "sp1", (300, 1, 1, 256, 132, 1, 1, 0)),
    Case("wgrad_bias", "wgrad.bias wgrad.lin wgrad.accumulate", "sp1", (2, 9, 9, 32, 64, 1, 1, 0), accumulate=True),
]

FAMILY = {"dgrad": "dgrad", "dgrad_gated": "dgrad", "dgrad_s1": "dgrad", "dgrad_gelu": "dgrad"}
for _e in ("wgrad", "wgrad_xf", "wgrad_dyin", "wgrad_bias"):
    FAMILY[_e] = "wgrad"
FWD_KERNEL = {"fwd", "stats", "xf", "gated", "s2add", "dyin", "dyin_s2add", "sumin", "gelu", "gelu_dact", "mulgrad", "gelugrad", "dgrad_s1"}


def documented_branches():
    """{(label, form)} from the module docstring's branch list."""
    out = set()
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+((?:(?:f32|sp1|sp2)\s+)+)(?:conv_mfma\.hip:[A-Za-z_]\w*|ops\.py)", line)
        if m:
            out |= {(m.group(1), f) for f in m.group(2).split()}
    return out


def defines(src, name):
    """Does the C++ text src hold a DEFINITION of function `name`: a declarator starting a line whose parameter list is followed by a body, not a `;`?"""
    for m in re.finditer(r"^[A-Za-z][^\n;{}()]*\b%s\(" % re.escape(name), src, re.M):
        depth, i = 1, m.end()
        while depth and i < len(src):
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        if re.match(r"\s*\{", src[i:]):
            return True
    return False


def covered_branches():
    out = set()
    for c in CASES:
        for b in c.branches:
            out.add((b, "f32"))
            out.add((b, c.form))
    return out


def test_case_table_covers_every_documented_branch():
    """GPU-free: every (branch, form) of the docstring has a case, every case's label names a documented branch, and the form labels follow the
    dispatch rule (forward-kernel launches: sp2 exactly when the contraction exceeds 1152)."""
    doc = documented_branches()
    assert len(doc) > 60
    missing = doc - covered_branches()
    assert not missing, f"documented branches without a case: {sorted(missing)}"
    labels = {b for b, _ in doc}
    stray = {b for c in CASES for b in c.branches} - labels
    assert not stray, f"cases name undocumented branches: {sorted(stray)}"
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "self-supervised-vision_amd", "csrc", "conv_mfma.hip")).read()
    named = set(re.findall(r"conv_mfma\.hip:([A-Za-z_]\w*)", __doc__))
    assert len(named) >= 10
    for name in sorted(named):
        assert defines(src, name), f"the docstring names conv_mfma.hip:{name}, which the source does not define"
    for c in CASES:
        n, h, w, ch, k, r, s, pad = c.geom
        if c.entry in FWD_KERNEL and c.form != "f32":
            contraction = r * r * (k if c.entry == "dgrad_s1" else ch)
            assert c.form == ("sp2" if contraction > 1152 else "sp1"), c.id
        if c.entry in ("wgrad", "wgrad_xf", "wgrad_dyin", "wgrad_bias"):
            assert c.form == ("sp1" if ch % 4 == 0 and k % 4 == 0 and ch != 3 else "f32"), c.id
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


# ============================================================================================================================ GPU helpers
def _lib():
    from ssv_amd import _lib as L
    return L


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib().load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_FORMS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


def _out(shape, dev, prior=None):
    """(buffer, view): the output as a view into a NaN-prefilled buffer with GUARD floats behind it; ``prior``: initial content of the output."""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    if prior is not None:
        buf[:n].copy_(prior.reshape(-1))
    return buf, buf[:n].view(shape)


def _guard_ok(buf, what):
    n = buf.numel() - GUARD
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} elements of the output never written"
    assert torch.isnan(buf[n:]).all(), f"{what}: wrote past the end of its output"


def _planes(t, keep):
    L = _lib()
    n = t.numel()
    assert n % 8 == 0
    pl = torch.empty((3, n), dtype=torch.int16, device=t.device)
    L.call("ssv_split_planes", n, L.ptr(t), L.ptr(pl), L.stream())
    keep.append(pl)
    return pl


def _desc(geom, arith, w=None, keep=None):
    """The descriptor of a launch; under bf16x3 the weight operand's planes ride along (when it has a whole number of 8-element groups)."""
    L = _lib()
    n, h, w_, c, k, r, s, pad = geom
    ho, wo = (h + 2 * pad - r) // s + 1, (w_ + 2 * pad - r) // s + 1
    d = L.ConvDesc(n, h, w_, c, k, r, r, s, pad, ho, wo)
    if arith == "bf16x3":
        d.arithmetic = L.ARITH_BF16X3
        if w is not None and w.numel() % 8 == 0:
            d.w_planes = _planes(w, keep).data_ptr()
    return d


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv64(x, w, s, pad):
    return F.conv2d(_nchw(x), _nchw(w), stride=s, padding=pad).permute(0, 2, 3, 1)


def _dgrad64(dy, w, xshape, s, pad):
    n, h, w_, c = xshape
    return torch.nn.grad.conv2d_input((n, c, h, w_), _nchw(w), _nchw(dy), stride=s, padding=pad).permute(0, 2, 3, 1)


def _wgrad64(x, dy, wshape, s, pad):
    k, r, r2, c = wshape
    return torch.nn.grad.conv2d_weight(_nchw(x), (k, c, r, r2), _nchw(dy), stride=s, padding=pad).permute(0, 2, 3, 1)


def _gelu64(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def _gelu_grad64(h):
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def _bits(mask, shape):
    """the ReLU byte mask (one byte per 4 consecutive elements, bit e = element 4 i + e) as a bool tensor of ``shape``"""
    return torch.stack([(mask >> e) & 1 for e in range(4)], dim=1).reshape(shape).bool()


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _bound_check(got, ref, amag, family, what):
    """(a): |got - ref| <= TAU * 2^-24 * A + floor."""
    err = (got.double() - ref).abs()
    floor = 1e-30 + 1e-3 * U * float(amag.max())
    bound = TAU[family] * U * amag + floor
    ratio = float((err / bound).max())
    WORST[family] = max(WORST.get(family, 0.0), ratio)              # worst |err| / bound per family (SSV_FORMS_REPORT)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err / bound).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements over the bound; worst at flat {i}: got {float(got.reshape(-1)[i]):.9g} "
                             f"ref {float(ref.reshape(-1)[i]):.9g} A {float(amag.reshape(-1)[i]):.3e} (|err| / bound = {ratio:.2f})")
    return ratio


def _group_check(got, rows_of_group, ngroups_api, val64, mag64, what):
    """(d): got [groups][ch] against the fp64 sums over the listed rows of val64 [rows][ch]; groups with no rows must be zero."""
    assert got.shape[0] == ngroups_api, f"{what}: {got.shape[0]} partial rows for {ngroups_api} groups"
    ref = torch.zeros(got.shape, dtype=torch.float64, device=got.device)
    mag = torch.zeros_like(ref)
    for g, idx in enumerate(rows_of_group):
        if idx is not None and idx.numel():
            ref[g] = val64[idx].sum(0)
            mag[g] = mag64[idx].sum(0)
    _bound_check(got, ref, mag, "partials", what)
    empty = [g for g, idx in enumerate(rows_of_group) if idx is None or idx.numel() == 0]
    if empty:
        assert (got[empty] == 0).all(), f"{what}: groups past the rows are not zero"


def _fwd_groups(m, count, dev):
    return [torch.arange(64 * g, min(64 * g + 64, m), device=dev) if 64 * g < m else None for g in range(count)]


def _dgrad_groups(n, h, w_, st, bm, count, dev):
    """row lists (flat NHW pixel indices) of the strided data gradient's gate partials: (parity class, row tile, 64-row group) - every class
    has as many row tiles as the largest one (class (0, 0))."""
    mc0 = n * (-(-h // st)) * (-(-w_ // st))
    per_class = -(-mc0 // bm) * (bm // 64)
    assert per_class * st * st == count
    out = []
    for cls in range(st * st):
        ph, pw = divmod(cls, st)
        hq, wq = len(range(ph, h, st)), len(range(pw, w_, st))
        nn_, hh, ww = torch.meshgrid(torch.arange(n), torch.arange(hq), torch.arange(wq), indexing="ij")
        pix = ((nn_ * h + hh * st + ph) * w_ + ww * st + pw).reshape(-1).to(dev)
        for j in range(per_class):
            sl = pix[64 * j:64 * j + 64]
            out.append(sl if sl.numel() else None)
    return out


class Run:
    """The outputs of one case in one arithmetic."""

    def __init__(self):
        self.outs = []          # (name, got, ref64, amag64, family, main)
        self.bufs = []          # (name, buffer) guarded outputs
        self.parts = []         # (name, got [groups][ch], rows per group, api count, val64, mag64)
        self.same = []          # (name, a, b) bitwise identities
        self.arith = []         # (product, desc) for ssv_conv_arithmetic


def _rand(g, *shape, scale=1.0, shift=0.0, dev=None):
    return torch.randn(*shape, device=dev, generator=g) * scale + shift


def _gate_ctx(g, kind, shape, dev):
    """x, mean, invstd, scale, shift, mask, x2, mean2, invstd2 for a gate on an output of ``shape``."""
    ch = shape[-1]
    x = _rand(g, *shape, scale=1.3, shift=0.2, dev=dev)
    mean, invstd = _rand(g, ch, scale=0.3, dev=dev), torch.rand(ch, device=dev, generator=g) + 0.5
    ctx = dict(x=x, mean=mean, invstd=invstd, scale=None, shift=None, mask=None, x2=None, mean2=None, invstd2=None)
    if kind == "affine":
        ctx["scale"] = torch.rand(ch, device=dev, generator=g) + 0.5
        ctx["shift"] = _rand(g, ch, scale=0.3, dev=dev)
    else:
        ctx["mask"] = torch.randint(0, 16, (math.prod(shape) // 4,), device=dev, generator=g, dtype=torch.uint8)
    if kind == "x2":
        ctx["x2"] = _rand(g, *shape, scale=0.7, shift=-0.2, dev=dev)
        ctx["mean2"], ctx["invstd2"] = _rand(g, ch, scale=0.2, dev=dev), torch.rand(ch, device=dev, generator=g) + 0.5
    return ctx


def _gate_bits(ctx, shape):
    if ctx["mask"] is not None:
        return _bits(ctx["mask"], shape)
    return (ctx["x"].double() * ctx["scale"].double() + ctx["shift"].double()) > 0        # the sign of fmaf(x, scale, shift): x * scale is exact in fp64


def _gate_struct(ctx, groups, ch, dev, run, name):
    L = _lib()
    n3 = 3 if ctx["x2"] is not None else 2
    bufs = [_out((groups, ch), dev) for _ in range(n3)]
    for i, (b, _) in enumerate(bufs):
        run.bufs.append((f"{name} partial {i}", b))
    P = L.ptr
    st = L.BnGate(P(ctx["x"]), P(ctx["scale"]), P(ctx["shift"]), P(ctx["mask"]), P(ctx["mean"]), P(ctx["invstd"]), P(bufs[0][1]), P(bufs[1][1]),
                  P(ctx["x2"]), P(ctx["mean2"]), P(ctx["invstd2"]), P(bufs[2][1]) if n3 == 3 else None)
    return st, [v for _, v in bufs]


def _gate_partials(run, ctx, parts, rows_of_group, count, gflat, name):
    """(d) for the gate: sum g, sum g * xhat (and sum g * xhat2) of the rows the kernel wrote."""
    g64 = gflat.double()
    ch = g64.shape[-1]
    xh = (ctx["x"].reshape(-1, ch).double() - ctx["mean"].double()) * ctx["invstd"].double()
    xm = (ctx["x"].reshape(-1, ch).double().abs() + ctx["mean"].double().abs()) * ctx["invstd"].double() * 2
    run.parts.append((f"{name} psum_g", parts[0], rows_of_group, count, g64, g64.abs()))
    run.parts.append((f"{name} psum_gx", parts[1], rows_of_group, count, g64 * xh, g64.abs() * xm))
    if ctx["x2"] is not None:
        xh2 = (ctx["x2"].reshape(-1, ch).double() - ctx["mean2"].double()) * ctx["invstd2"].double()
        xm2 = (ctx["x2"].reshape(-1, ch).double().abs() + ctx["mean2"].double().abs()) * ctx["invstd2"].double() * 2
        run.parts.append((f"{name} psum_gx2", parts[2], rows_of_group, count, g64 * xh2, g64.abs() * xm2))


def _stats_partials(run, pm, p2, y, m, k, count):
    """(d) for the statistics epilogue: per 64-row group, the mean and the centred sum of squares of the rows written (the kernel sums around the
    group's first row: its error scales with sum (y - y0)^2)."""
    y64 = y.reshape(m, k).double()
    rows = _fwd_groups(m, count, y.device)
    ref_m, mag_m = torch.zeros(count, k, dtype=torch.float64, device=y.device), torch.zeros(count, k, dtype=torch.float64, device=y.device)
    ref_2, mag_2 = torch.zeros_like(ref_m), torch.zeros_like(ref_m)
    for g, idx in enumerate(rows):
        blk = y64[idx]
        mu = blk.mean(0)
        ref_m[g], mag_m[g] = mu, blk[0].abs() + (blk - blk[0]).abs().mean(0)
        ref_2[g], mag_2[g] = ((blk - mu) ** 2).sum(0), ((blk - blk[0]) ** 2).sum(0) * 2
    run.outs.append(("pmean", pm, ref_m, mag_m, "partials", False))
    run.outs.append(("pm2", p2, ref_2, mag_2, "partials", False))


# ============================================================================================================================ the runners
def _run_fwd_family(case, arith, dev):
    """Every forward-kernel entry point: returns a Run."""
    L = _lib()
    P = L.ptr
    e, o = case.entry, case.opt
    n, h, w_, c, k, r, s, pad = case.geom
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(case.id.encode()))
    run, keep = Run(), []
    ho, wo = (h + 2 * pad - r) // s + 1, (w_ + 2 * pad - r) // s + 1
    m, mi = n * ho * wo, n * h * w_
    x = _rand(g, n, h, w_, c, dev=dev)
    w = _rand(g, k, r, r, c, scale=(1.0 / (r * r * c)) ** 0.5, dev=dev)
    x64, w64 = x.double(), w.double()
    yshape = (n, ho, wo, k)
    d = _desc(case.geom, arith, w, keep)
    run.arith.append((0, d))
    stream = L.stream()

    if e == "fwd":
        bias = _rand(g, k, dev=dev) if o.get("bias") else None
        add = _rand(g, *yshape, dev=dev) if o.get("addend") else None
        buf, y = _out(yshape, dev)
        L.call("ssv_conv2d_fwd", C.byref(d), P(x), P(w), P(bias), P(add), P(y), stream)
        ref, amag = _conv64(x64, w64, s, pad), _conv64(x64.abs(), w64.abs(), s, pad)
        if bias is not None:
            ref, amag = ref + bias.double(), amag + bias.double().abs()
        if add is not None:
            ref, amag = ref + add.double(), amag + add.double().abs()
        run.outs.append(("y", y, ref, amag, "fwd", True))
        run.bufs.append(("y", buf))
        return run, keep

    if e in ("stats", "xf"):
        sc = sh = None
        opnd, opnd_mag = x64, x64.abs()
        if e == "xf":
            sc, sh = torch.rand(c, device=dev, generator=g) + 0.5, _rand(g, c, scale=0.5, dev=dev)
            pre = x64 * sc.double() + sh.double()
            opnd = torch.relu(pre)
            opnd_mag = (x64 * sc.double()).abs() + sh.double().abs()
            opnd_mag = torch.where(pre > 0, opnd_mag, torch.zeros_like(opnd_mag))
        stats = e == "stats" or o.get("stats")
        groups = int(L.load().ssv_conv2d_fwd_stats_groups(C.byref(d)))
        assert groups == -(-m // 64)
        buf, y = _out(yshape, dev)
        run.bufs.append(("y", buf))
        pm = p2 = None
        if stats:
            (bm_, pm), (b2_, p2) = _out((groups, k), dev), _out((groups, k), dev)
            run.bufs += [("pmean", bm_), ("pm2", b2_)]
        if e == "stats":
            L.call("ssv_conv2d_fwd_stats", C.byref(d), P(x), P(w), P(y), P(pm), P(p2), stream)
        else:
            L.call("ssv_conv2d_fwd_bnrelu_in_stats", C.byref(d), P(x), P(sc), P(sh), P(w), P(y), P(pm), P(p2), stream)
        run.outs.append(("y", y, _conv64(opnd, w64, s, pad), _conv64(opnd_mag, w64.abs(), s, pad), "fwd", True))
        if stats:
            _stats_partials(run, pm, p2, y, m, k, groups)
        # (f): the plain forward on the materialised operand (ssv_bn_apply: the same fmaf / fmaxf) gives the same bits
        xin = x
        if e == "xf":
            from ssv_amd import ops
            xin, _ = ops.bn_apply(x, sc, sh, relu=True)
        y_plain = torch.empty(yshape, device=dev)
        L.call("ssv_conv2d_fwd", C.byref(d), P(xin), P(w), None, None, P(y_plain), stream)
        run.same.append(("fused forward vs plain forward on the materialised operand", y, y_plain))
        return run, keep

    if e == "sumin":
        res = _rand(g, n, h, w_, c, dev=dev)
        sc, sh = torch.rand(c, device=dev, generator=g) + 0.5, _rand(g, c, scale=0.3, dev=dev)
        rsc = rsh = None
        if o.get("raff"):
            rsc, rsh = torch.rand(c, device=dev, generator=g) + 0.5, _rand(g, c, scale=0.3, dev=dev)
        groups = int(L.load().ssv_conv2d_fwd_stats_groups(C.byref(d)))
        (by, y), (bpm, pm), (bp2, p2), (ba, a) = _out(yshape, dev), _out((groups, k), dev), _out((groups, k), dev), _out((n, h, w_, c), dev)
        run.bufs += [("y", by), ("pmean", bpm), ("pm2", bp2), ("a_out", ba)]
        mask = None
        if o.get("mask"):
            mbuf = torch.full((mi * c // 4 + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
            mask = mbuf[:mi * c // 4]
        L.call("ssv_conv2d_fwd_sumin_stats", C.byref(d), P(x), P(res), P(sc), P(sh), P(rsc), P(rsh), P(w), P(y), P(pm), P(p2), P(a), P(mask), stream)
        r64 = res.double() if rsc is None else res.double() * rsc.double() + rsh.double()
        rmag = res.double().abs() if rsc is None else (res.double() * rsc.double()).abs() + rsh.double().abs()
        pre = x64 * sc.double() + sh.double() + r64
        a64 = torch.relu(pre)
        amag_a = (x64 * sc.double()).abs() + sh.double().abs() + rmag
        run.outs.append(("a_out", a, a64, amag_a, "fwd", False))
        # the operand the GEMM saw is the kernel's own a (its ReLU decision may differ from fp64's at a rounding-level boundary): the product is checked on it
        run.outs.append(("y", y, _conv64(a.double(), w64, 1, 0), _conv64(a.double().abs(), w64.abs(), 1, 0), "fwd", True))
        _stats_partials(run, pm, p2, y, m, k, groups)
        from ssv_amd import ops
        a_ref, m_ref = ops.bn_apply(x, sc, sh, relu=True, residual=res, res_affine=None if rsc is None else (rsc, rsh), want_mask=True)
        run.same.append(("a_out vs ssv_bn_apply", a, a_ref))
        if mask is not None:
            run.same.append(("mask_out vs ssv_bn_apply", mask, m_ref))
            assert (mbuf[mi * c // 4:] == 0xA5).all(), "mask_out written past its end"
        y2, pm2_, p22 = torch.empty_like(y), torch.empty_like(pm), torch.empty_like(p2)
        L.call("ssv_conv2d_fwd_stats", C.byref(d), P(a_ref), P(w), P(y2), P(pm2_), P(p22), stream)
        run.same += [("y vs bn_apply + fwd_stats", y, y2), ("pmean vs bn_apply + fwd_stats", pm, pm2_), ("pm2 vs bn_apply + fwd_stats", p2, p22)]
        return run, keep

    if e in ("gated", "s2add", "dyin", "dyin_s2add"):
        add = None
        h2 = w2 = 0
        if e in ("s2add", "dyin_s2add"):
            h2, w2 = (ho + 1) // 2, (wo + 1) // 2
            add = _rand(g, n, h2, w2, k, dev=dev)
            full = torch.zeros(yshape, dtype=torch.float64, device=dev)
            full[:, ::2, ::2, :] = add.double()
            add64 = full
        elif o.get("addend"):
            add = _rand(g, *yshape, dev=dev)
            add64 = add.double()
        else:
            add64 = torch.zeros(yshape, dtype=torch.float64, device=dev)
        opnd, opnd_mag, src = x64, x64.abs(), x
        dyin = None
        if e in ("dyin", "dyin_s2add"):
            xb = _rand(g, n, h, w_, c, scale=1.7, shift=0.6, dev=dev)
            coef = torch.stack([torch.rand(c, device=dev, generator=g) + 0.25, _rand(g, c, scale=0.5, dev=dev) + 0.6,
                                _rand(g, c, scale=0.2, dev=dev), _rand(g, c, scale=0.05, dev=dev)]).contiguous()
            cf = coef.double()
            xc = xb.double() - cf[1]
            opnd = x64 * cf[0] + xc * cf[2] + cf[3]
            opnd_mag = (x64 * cf[0]).abs() + (xc * cf[2]).abs() + cf[3].abs()
            dyin = L.BnDyin(P(xb), P(coef))
            keep += [xb, coef]
        kind = o.get("gate")
        ctx = _gate_ctx(g, kind, yshape, dev) if kind else None
        buf, y = _out(yshape, dev)
        run.bufs.append(("y", buf))
        count, st, parts = 0, None, None
        if ctx is not None:
            count = int(L.load().ssv_conv2d_fwd_gate_groups(C.byref(d)))
            bm = 128 if (k >= 128 or case.form != "f32" and arith == "bf16x3") else 256
            assert count == -(-m // bm) * (bm // 64), (count, bm)
            st, parts = _gate_struct(ctx, count, k, dev, run, "gate")
        if e == "gated":
            L.call("ssv_conv2d_fwd_gated", C.byref(d), P(x), P(w), P(add), P(y), C.byref(st), stream)
        elif e == "s2add":
            L.call("ssv_conv2d_fwd_gated_s2add", C.byref(d), P(x), P(w), P(add), h2, w2, P(y), C.byref(st), stream)
        elif e == "dyin":
            L.call("ssv_conv2d_fwd_dyin", C.byref(d), P(src), C.byref(dyin), P(w), P(add), P(y), None if st is None else C.byref(st), stream)
        else:
            L.call("ssv_conv2d_fwd_dyin_s2add", C.byref(d), P(src), C.byref(dyin), P(w), P(add), h2, w2, P(y), C.byref(st), stream)
        ref = _conv64(opnd, w64, s, pad) + add64
        amag = _conv64(opnd_mag, w64.abs(), s, pad) + add64.abs()
        if ctx is not None:
            bits = _gate_bits(ctx, yshape)
            ref, amag = torch.where(bits, ref, 0.0), torch.where(bits, amag, 0.0)
            _gate_partials(run, ctx, parts, _fwd_groups(m, count, dev), count, y.reshape(m, k), "gate")
        run.outs.append(("y", y, ref, amag, "fwd", True))
        if e == "gated":
            # (f): the gated output is the plain forward (+ addend) with the gate's zeros
            y_plain = torch.empty(yshape, device=dev)
            L.call("ssv_conv2d_fwd", C.byref(d), P(x), P(w), None, P(add), P(y_plain), stream)
            run.same.append(("gated vs masked plain forward", y, torch.where(_gate_bits(ctx, yshape), y_plain, torch.zeros((), device=dev))))
        return run, keep

    # the Linear + GELU products: rows M = n, contraction c, outputs k; the weight operand [k][c]
    assert r == 1 and h == 1 and w_ == 1
    xm, wm = x.reshape(n, c), w.reshape(k, c)
    lin64, linmag = xm.double() @ wm.double().t(), xm.double().abs() @ wm.double().abs().t()
    if e in ("gelu", "gelu_dact"):
        bias = _rand(g, k, dev=dev)
        hh, hmag = lin64 + bias.double(), linmag + bias.double().abs()
        (ba, act), (bh, hout) = _out((n, k), dev), _out((n, k), dev)
        run.bufs.append(("act", ba))
        if e == "gelu":
            keep_h = o.get("keep_h")
            if keep_h:
                run.bufs.append(("h", bh))
            L.call("ssv_linear_gelu_fwd", C.byref(d), P(xm), P(wm), P(bias), P(hout) if keep_h else None, P(act), stream)
            if keep_h:
                run.outs.append(("h", hout, hh, hmag, "fwd", True))
        else:
            run.bufs.append(("dact", bh))
            L.call("ssv_linear_gelu_fwd_dact", C.byref(d), P(xm), P(wm), P(bias), P(hout), P(act), stream)
            run.outs.append(("dact", hout, _gelu_grad64(hh), 0.8 * hmag + 1.0, "fwd", True))
        # gelu' <= 1.13, gelu'' <= 0.8: the activation / derivative inherit the pre-activation's bound, plus the evaluation's own rounding
        run.outs.append(("act", act, _gelu64(hh), 1.13 * hmag + hh.abs(), "fwd", e == "gelu" and not o.get("keep_h")))
        return run, keep
    # mulgrad / gelugrad: dh = (dy wt^T) * factor (+ addend), dy = x [n][c], wt = w [k][c]
    hpre = _rand(g, n, k, dev=dev)
    fac = None
    if e == "mulgrad":
        fac = _rand(g, n, k, scale=0.5, shift=0.5, dev=dev)
        f64 = fac.double()
    else:
        f64 = _gelu_grad64(hpre.double())
    add = _rand(g, n, k, dev=dev) if o.get("addend") else None
    buf, dh = _out((n, k), dev)
    run.bufs.append(("dh", buf))
    if e == "mulgrad":
        L.call("ssv_linear_fwd_mulgrad", C.byref(d), P(xm), P(wm), P(fac), P(add), P(dh), stream)
    else:
        L.call("ssv_linear_fwd_gelugrad", C.byref(d), P(xm), P(wm), P(hpre), P(add), P(dh), stream)
    ref, amag = lin64 * f64, linmag * f64.abs() + (0 if e == "mulgrad" else lin64.abs())        # gelu'(h) evaluated in fp32: a few ulps of 1
    if add is not None:
        ref, amag = ref + add.double(), amag + add.double().abs()
    run.outs.append(("dh", dh, ref, amag, "fwd", True))
    return run, keep


def _run_dgrad(case, arith, dev):
    L = _lib()
    P = L.ptr
    e, o = case.entry, case.opt
    n, h, w_, c, k, r, s, pad = case.geom
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(case.id.encode()))
    run, keep = Run(), []
    ho, wo = (h + 2 * pad - r) // s + 1, (w_ + 2 * pad - r) // s + 1
    dy = _rand(g, n, ho, wo, k, dev=dev)
    w = _rand(g, k, r, r, c, scale=(1.0 / (r * r * k)) ** 0.5, dev=dev)
    xshape = (n, h, w_, c)
    stream = L.stream()
    if e == "dgrad_gelu":                               # a Linear: rows n, inputs c, outputs k
        hpre = _rand(g, n, c, dev=dev)
        add = _rand(g, n, c, dev=dev) if o.get("addend") else None
        d = _desc(case.geom, arith)                     # as ops.linear_dgrad_gelu: no planes (the kernel has no bf16-piece form)
        run.arith.append((1, d))
        buf, dx = _out((n, c), dev)
        run.bufs.append(("dx", buf))
        L.call("ssv_conv2d_dgrad_gelu", C.byref(d), P(dy), P(w), P(hpre), P(add), P(dx), stream)
        lin, linmag = dy.reshape(n, k).double() @ w.reshape(k, c).double(), dy.reshape(n, k).double().abs() @ w.reshape(k, c).double().abs()
        f64 = _gelu_grad64(hpre.double())
        ref, amag = lin * f64, linmag * f64.abs() + lin.abs()
        if add is not None:
            ref, amag = ref + add.double(), amag + add.double().abs()
        run.outs.append(("dx", dx, ref, amag, "dgrad", True))
        return run, keep
    ref = _dgrad64(dy.double(), w.double(), xshape, s, pad)
    amag = _dgrad64(dy.double().abs(), w.double().abs(), xshape, s, pad)
    if e == "dgrad_s1":
        from ssv_amd import ops
        add = _rand(g, *xshape, dev=dev) if o.get("addend") else None
        wc = w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        dx = ops.conv2d_dgrad(dy, wc, xshape, 1, pad, addend=add)
        # the launch ops made: the forward kernel on the transposed filter (contraction over k)
        wt = ops._transposed_filter(wc, (k, c, r, r))
        run.arith.append((0, _desc((n, ho, wo, k, c, r, 1, r - 1 - pad), arith, wt, keep)))
        if add is not None:
            ref, amag = ref + add.double(), amag + add.double().abs()
        run.outs.append(("dx", dx, ref, amag, "dgrad", True))
        return run, keep
    d = _desc(case.geom, arith, w, keep)
    run.arith.append((1, d))
    add = o.get("addend")
    prior = _rand(g, *xshape, dev=dev) if add else None
    buf, dx = _out(xshape, dev, prior if add == "alias" else None)
    run.bufs.append(("dx", buf))
    addp = None if not add else (dx if add == "alias" else prior)
    if prior is not None:
        ref, amag = ref + prior.double(), amag + prior.double().abs()
    kind = o.get("gate")
    if e == "dgrad":
        L.call("ssv_conv2d_dgrad", C.byref(d), P(dy), P(w), P(addp), P(dx), stream)
    else:
        ctx = _gate_ctx(g, kind, xshape, dev)
        count = int(L.load().ssv_conv2d_dgrad_gate_groups(C.byref(d)))
        bm = 128 if c >= 128 else 256
        st, parts = _gate_struct(ctx, count, c, dev, run, "gate")
        L.call("ssv_conv2d_dgrad_gated", C.byref(d), P(dy), P(w), P(addp), P(dx), C.byref(st), stream)
        bits = _gate_bits(ctx, xshape)
        ref, amag = torch.where(bits, ref, 0.0), torch.where(bits, amag, 0.0)
        _gate_partials(run, ctx, parts, _dgrad_groups(n, h, w_, s, bm, count, dev), count, dx.reshape(-1, c), "gate")
        dx_plain = torch.empty(xshape, device=dev)
        L.call("ssv_conv2d_dgrad", C.byref(d), P(dy), P(w), P(prior), P(dx_plain), stream)
        run.same.append(("gated vs masked plain data gradient", dx, torch.where(bits, dx_plain, torch.zeros((), device=dev))))
    run.outs.append(("dx", dx, ref, amag, "dgrad", True))
    return run, keep


def _wgrad_plan(case):
    """nsplit and chunk rows of plan_wgrad (conv_mfma.hip) for a plain weight gradient."""
    n, h, w_, c, k, r, s, pad = case.geom
    ho, wo = (h + 2 * pad - r) // s + 1, (w_ + 2 * pad - r) // s + 1
    m, rsc = n * ho * wo, r * r * c
    bm, bn = (128 if k >= 128 else 64), (64 if rsc <= 64 else 128)
    tiles = -(-k // bm) * -(-rsc // bn)
    ns = max(1, min((768 if bm == 128 else 1024) // tiles, -(-m // 256)))
    chunk = -(-(-(-m // ns)) // 32) * 32
    return m, -(-m // chunk), chunk


def _run_wgrad(case, arith, dev):
    L = _lib()
    P = L.ptr
    e, o = case.entry, case.opt
    n, h, w_, c, k, r, s, pad = case.geom
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(case.id.encode()))
    run, keep = Run(), []
    ho, wo = (h + 2 * pad - r) // s + 1, (w_ + 2 * pad - r) // s + 1
    x = _rand(g, n, h, w_, c, dev=dev)
    dy = _rand(g, n, ho, wo, k, dev=dev)
    d = _desc(case.geom, arith)
    run.arith.append((2, d))
    stream = L.stream()
    x64, xmag = x.double(), x.double().abs()
    sc = sh = None
    if e == "wgrad_xf" or o.get("in_affine"):
        sc, sh = torch.rand(c, device=dev, generator=g) + 0.5, _rand(g, c, scale=0.5, dev=dev)
        pre = x64 * sc.double() + sh.double()
        x64 = torch.relu(pre)
        xmag = torch.where(pre > 0, (x.double() * sc.double()).abs() + sh.double().abs(), 0.0)
    dy64, dymag = dy.double(), dy.double().abs()
    dyin = None
    if e == "wgrad_dyin":
        xb = _rand(g, n, ho, wo, k, scale=1.7, shift=0.6, dev=dev)
        coef = torch.stack([torch.rand(k, device=dev, generator=g) + 0.25, _rand(g, k, scale=0.5, dev=dev) + 0.6,
                            _rand(g, k, scale=0.2, dev=dev), _rand(g, k, scale=0.05, dev=dev)]).contiguous()
        cf = coef.double()
        xc = xb.double() - cf[1]
        dy64 = dy.double() * cf[0] + xc * cf[2] + cf[3]
        dymag = (dy.double() * cf[0]).abs() + (xc * cf[2]).abs() + cf[3].abs()
        dyin = L.BnDyin(P(xb), P(coef))
        keep += [xb, coef]
    wshape = (k, r, r, c)
    ref, amag = _wgrad64(x64, dy64, wshape, s, pad), _wgrad64(xmag, dymag, wshape, s, pad)
    acc = bool(o.get("accumulate"))
    prior = _rand(g, *wshape, dev=dev) if acc else None
    buf, dw = _out(wshape, dev, prior)
    run.bufs.append(("dw", buf))
    if acc:
        ref, amag = ref + prior.double(), amag + prior.double().abs()
    lib = L.load()
    if e == "wgrad_bias":
        wsb = int(lib.ssv_conv2d_wgrad_bias_workspace_bytes(C.byref(d)))
        ws = torch.empty(wsb // 4 + 4, device=dev)
        bprior = _rand(g, k, dev=dev) if acc else None
        bbuf, db = _out((k,), dev, bprior)
        run.bufs.append(("dbias", bbuf))
        L.call("ssv_conv2d_wgrad_bias", C.byref(d), P(x), P(dy), P(dw), P(db), int(acc), P(ws), wsb, stream)
        bref, bmag = dy.double().reshape(-1, k).sum(0), dy.double().abs().reshape(-1, k).sum(0)
        if acc:
            bref, bmag = bref + bprior.double(), bmag + bprior.double().abs()
        run.outs.append(("dbias", db, bref, bmag, "wgrad", False))
    else:
        wsb = int(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d)))
        m, nsplit, chunk = _wgrad_plan(case)
        assert wsb == nsplit * k * r * r * c * 4, "plan_wgrad changed: update _wgrad_plan"
        if "wgrad.nsplit_ragged" in case.branches:
            assert nsplit > 1 and m % chunk != 0, (m, nsplit, chunk)
        ws = torch.empty(wsb // 4 + 4, device=dev)
        if e == "wgrad_dyin":
            L.call("ssv_conv2d_wgrad_dyin", C.byref(d), P(x), P(sc), P(sh), P(dy), C.byref(dyin), P(dw), int(acc), P(ws), wsb, stream)
        else:
            L.call("ssv_conv2d_wgrad_bnrelu_in", C.byref(d), P(x), P(sc), P(sh), P(dy), P(dw), int(acc), P(ws), wsb, stream)
    run.outs.append(("dw", dw, ref, amag, "wgrad", True))
    if e == "wgrad_xf":
        from ssv_amd import ops
        xa, _ = ops.bn_apply(x, sc, sh, relu=True)
        dw2 = torch.empty(wshape, device=dev) if not acc else prior.clone()
        ws2 = torch.empty(int(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d))) // 4 + 4, device=dev)
        L.call("ssv_conv2d_wgrad", C.byref(d), P(xa), P(dy), P(dw2), int(acc), P(ws2), ws2.numel() * 4, stream)
        run.same.append(("formed-on-load weight gradient vs plain on the materialised operand", dw, dw2))
    return run, keep


def _run(case, arith, dev):
    from ssv_amd import ops
    with ops.arithmetic(arith):
        if case.entry.startswith("wgrad"):
            out = _run_wgrad(case, arith, dev)
        elif case.entry in ("dgrad", "dgrad_gated", "dgrad_s1", "dgrad_gelu"):
            out = _run_dgrad(case, arith, dev)
        else:
            out = _run_fwd_family(case, arith, dev)
        torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_launch_form_against_fp64_in_both_arithmetics(dev, case):
    L = _lib()
    lib = L.load()
    runs = {}
    for arith in ("f32", "bf16x3"):
        run, keep = _run(case, arith, dev)
        runs[arith] = run
        what = f"{case.id} [{arith}]"
        # (c) the launched arithmetic
        want = L.ARITH_BF16X3 if (arith == "bf16x3" and case.form != "f32") else L.ARITH_F32_MFMA
        for product, d in run.arith:
            assert lib.ssv_conv_arithmetic(C.byref(d), product) == want, f"{what}: ssv_conv_arithmetic(product {product}) is not {case.form}"
        # (e) guards
        for name, buf in run.bufs:
            _guard_ok(buf, f"{what} {name}")
        # (a) element-wise bounds
        for name, got, ref, amag, fam, _ in run.outs:
            _bound_check(got, ref, amag, fam, f"{what} {name}")
        # (d) partial sums
        for name, got, rows, count, val, mag in run.parts:
            _group_check(got, rows, count, val, mag, f"{what} {name}")
        # (f) bitwise identities
        for name, a, b in run.same:
            assert torch.equal(a, b), f"{what}: {name} not bit-identical (max |diff| {float((a.double() - b.double()).abs().max()):.3e})"
        del keep
    # (b) the two arithmetics against fp64
    for (name, g32, ref, _, _, main), (_, gsp, _, _, _, _) in zip(runs["f32"].outs, runs["bf16x3"].outs):
        if not main:
            continue
        if case.form == "f32":
            assert torch.equal(g32, gsp), f"{case.id} {name}: no bf16-piece form, yet the two arithmetics differ"
        else:
            e32, esp = _rel(g32, ref), _rel(gsp, ref)
            bar = SPARSE_SP1_BAR if (case.entry in ("xf", "sumin") and case.form == "sp1") else 1.05
            assert esp <= bar * e32 + 1e-9, f"{case.id} {name}: bf16x3 {esp:.3e} vs fp32 MFMA {e32:.3e} against fp64 (bar {bar}x)"


# ============================================================================================================================ the plane-offset limit
@pytest.mark.gpu
@pytest.mark.parametrize("k,want", [(22528, "f32"), (21824, "bf16x3")])
def test_weights_whose_planes_exceed_2_gib_run_on_fp32(dev, k, want):
    """The bf16-piece kernels address the three planes of a weight with 32-bit byte offsets (6 K R S C bytes); check_desc admits K R S C up to 2^29.
    From 6 K R S C >= 2^31 (K = 22,528 x C = 16,384) the launch must take fp32 MFMA - a Linear and a 1x1 / stride-2 strided data gradient, against fp64;
    just below (K = 21,824) the bf16x3 form stays and is right too."""
    L = _lib()
    P = L.ptr
    lib = L.load()
    c, rows = 16384, 8
    g = torch.Generator(device=dev).manual_seed(7)
    w = _rand(g, k, c, scale=c ** -0.5, dev=dev)
    x = _rand(g, rows, c, dev=dev)
    dy = _rand(g, 1, 2, 2, k, dev=dev)
    want_code = L.ARITH_BF16X3 if want == "bf16x3" else L.ARITH_F32_MFMA
    keep = []
    pl = _planes(w, keep)
    d = L.ConvDesc(rows, 1, 1, c, k, 1, 1, 1, 0, 1, 1)
    d.arithmetic, d.w_planes = L.ARITH_BF16X3, pl.data_ptr()
    dd = L.ConvDesc(1, 4, 4, c, k, 1, 1, 2, 0, 2, 2)
    dd.arithmetic, dd.w_planes = L.ARITH_BF16X3, pl.data_ptr()
    assert lib.ssv_conv_arithmetic(C.byref(d), 0) == want_code
    assert lib.ssv_conv_arithmetic(C.byref(dd), 1) == want_code
    yb, y = _out((rows, k), dev)
    L.call("ssv_conv2d_fwd", C.byref(d), P(x), P(w), None, None, P(y), L.stream())
    xb, dx = _out((1, 4, 4, c), dev)
    L.call("ssv_conv2d_dgrad", C.byref(dd), P(dy), P(w), None, P(dx), L.stream())
    torch.cuda.synchronize()
    del keep, pl
    _guard_ok(yb, "linear")
    _guard_ok(xb, "strided data gradient")
    ref, amag = torch.zeros(rows, k, dtype=torch.float64, device=dev), torch.zeros(rows, k, dtype=torch.float64, device=dev)
    dref, dmag = torch.zeros(4, c, dtype=torch.float64, device=dev), torch.zeros(4, c, dtype=torch.float64, device=dev)
    dyf = dy.reshape(4, k)
    for k0 in range(0, k, 4096):
        wc = w[k0:k0 + 4096].double()
        ref[:, k0:k0 + 4096] = x.double() @ wc.t()
        amag[:, k0:k0 + 4096] = x.double().abs() @ wc.abs().t()
        dref += dyf[:, k0:k0 + 4096].double() @ wc
        dmag += dyf[:, k0:k0 + 4096].double().abs() @ wc.abs()
        del wc
    _bound_check(y, ref, amag, "fwd", f"Linear {c} -> {k} [{want}]")
    full = torch.zeros(1, 4, 4, c, dtype=torch.float64, device=dev)
    fmag = torch.zeros_like(full)
    full[:, ::2, ::2, :], fmag[:, ::2, ::2, :] = dref.view(1, 2, 2, c), dmag.view(1, 2, 2, c)
    _bound_check(dx, full, fmag, "dgrad", f"1x1 / stride-2 data gradient {k} -> {c} [{want}]")
