"""Every BatchNorm, pooling and layout kernel between the convolutions (csrc/bn.hip, csrc/pool.hip: 21 launching entry points) against an fp64
evaluation of the same operation on the same fp32 inputs.

Each case of CASES names the entry points it reaches (straight through the C ABI, workspaces sized by ssv_bn_workspace_bytes and guarded; through
nn.* / ops.* only where the host composes several calls), the branch labels it targets and a shape.  The inputs are drawn on the CPU from a generator
seeded by the case id, so the GPU-free tests below see exactly what the GPU tests upload.  Every run is held to:

  (a) for every tensor a case produces, with ref64 = plain torch in float64 on the CPU of the written-out operation (BatchNorm as mean / centred
      variance / scale = gamma * invstd, shift = beta - mean * scale / y = x * scale + shift: the operation the ABI defines), ref32 = the SAME lines in
      float32 on the CPU, e(x) = ||x - ref64||_2 / ||ref64||_2 and m(x) = max|x - ref64| / max|ref64|:
          e(got) <= FACTOR[family] * e(ref32) + FLOOR[family]     and the same for m.
      e(ref32) comes from the reference, never from the library.  eps and momentum enter both references as the fp32 value the kernel receives.
      Families: bn-forward, bn-backward, reduction; outputs of the family `exact` (max-pool forward and arg-max, max-pool backward where a pixel
      receives at most one term, layouts, pad, group, filter transpose, the ReLU byte mask) must be bit-identical to ref32;
  (b) a condition on the inputs: ref64 is finite and not identically zero, ref32 is within 1e-3 of it (e and m) - test_reference_is_well_conditioned;
  (b') ReLU gates.  A gate that fp32 and fp64 decide differently makes the case measure nothing.  Where scale and shift are INPUTS (ssv_bn_apply,
      ssv_bn_relu_bwd_affine, both stem kernels) the gate of ref64 AND ref32 is x.double() * scale.double() + shift.double() > 0, whose sign is the sign
      of the kernel's fmaf; where y or a byte mask is an input (ssv_bn_train_bwd) the gate is data, handed to kernel and references alike; where the
      kernel computes the statistics itself (ssv_bn_train_fwd / _partials with ReLU, and ssv_bn_apply with a residual, whose add rounds a second time)
      the inputs are nudged: every element whose fp64 pre-activation a has |a| < TAU = 2^-14 is moved to |a| = 4 TAU on its own side.  Asserted
      GPU-free: no element inside TAU after at most two passes, max|a32 - a64| <= TAU / 4, zero gate flips.  On the GPU the written mask must then
      equal the fp64 gate exactly;
  (c) max-pool backward: dy scattered by the forward's arg-max; a pixel that collects up to four terms is under the bn-backward bar, one that collects
      at most one is exact.  The stem backward takes its arg-max (and xmax) as data: the fp64 forward's;
  (d) every output is a 16-byte aligned view into a NaN-prefilled buffer with 1024 floats of guard behind it (4096 behind a workspace): no output
      element stays NaN (pool.nonfinite excepted), the guard is untouched, every input is bit-identical afterwards; running_mean, running_var,
      num_batches_tracked and dgamma / dbeta / out under accumulate are the documented read-modify-write arguments;
  (e) the bitwise identities the sources state: ssv_bn_train_fwd_partials == ssv_bn_stats_finalize + ssv_bn_apply; ssv_bn_train_bwd from the byte
      mask == from y; ssv_bn_relu_bwd_affine == ssv_bn_train_bwd on the y ssv_bn_apply wrote; ssv_bn_relu_maxpool_fwd == ssv_bn_apply(relu) +
      ssv_maxpool3x3s2_fwd; ssv_bn_relu_maxpool_bwd without xmax == ssv_maxpool3x3s2_bwd + ssv_bn_train_bwd, with xmax within FACTOR * e(ref32) of
      it; ssv_bn_bwd_coef's dgamma / dbeta == ssv_bn_bwd_from_partials's; accumulate on a zero prior == overwrite; a second call == the first.

FACTOR and FLOOR: FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured per family on an MI355X
(profiles/bn_pool_kernels_report.json, written by this file under SSV_BNPOOL_REPORT=<path>), rounded up to the next power of two and never above 8.

bn_plan / apply_grid / merge_plan of csrc/bn_plan.h are restated below; test_restated_plan_is_the_plan_of_bn_plan_h holds the restatement to the C++ (a
stand-alone host program under ASan + UBSan), and test_case_shapes_have_the_property_their_label_claims holds every case to
the property its label names, so a retuned plan fails here instead of silently hollowing the table out.

Branch labels (label, entry point, what the case reaches) - test_case_table_covers_every_documented_branch keeps CASES honest:

  plan.min_rows        ssv_bn_train_fwd              C 64, M 1800: rows per block = 4 * RT
  plan.rpb_grows       ssv_bn_train_fwd              C 64, M 200003: rpb 196, 1021 blocks, ragged last block of 83 rows
  plan.idle_lanes      ssv_bn_train_fwd              C 96 (RT 10) and C 132 (RT 7): 256 % CT != 0
  plan.c4              ssv_bn_train_fwd              C 4: CT 1, RT 256, M 5 (fewer rows than RT) and M 3000
  plan.gy2             ssv_bn_train_fwd              C 2048, M 5000: GY 2, apply grid (512 blocks, rpb 10) != statistics grid (rpb 5)
  plan.gy_ragged       ssv_bn_train_fwd              C 1028: the second y-block has one live channel group
  plan.unroll_tail     ssv_bn_train_fwd              rows per lane 4k+1, 4k+2, 4k+3 and < 4
  stats.offset         ssv_bn_train_fwd              mean / std = 1000 (30 +- 0.03), no ReLU: the shifted sums; dx of ssv_bn_train_bwd relu 0
  stats.m1             ssv_bn_train_fwd              M 1: var 0, unbiased falls back to var, mean == x, y == beta under (a), dx (and an overwritten dgamma) == 0 exactly
  stats.running        ssv_bn_train_fwd              running statistics on a seeded prior, momentum 0.1 and 1.0, num_batches_tracked + 1; both NULL
  partials.one_level   ssv_bn_train_fwd_partials     <= 2048 groups, ragged last group, rows per group 1 (pm2 == 0) and 64
  partials.own_partition ssv_bn_train_fwd_partials   rows per group = bn_plan's rows per block (bn_stats_k's own partition): next to ssv_bn_train_fwd on the same input
  partials.factor32    ssv_bn_train_fwd_partials     > 2048 groups with cdiv(groups, 32) <= cap: M 200000 (3125 groups) and M 140003 (ragged last group)
  partials.factor_cap  ssv_bn_train_fwd_partials     > 2048 groups with cdiv(groups, 32) > cap: M 5000, C 8, 1 row per group (cap 10, factor 500)
  apply.res0           ssv_bn_apply                  no residual, with and without ReLU, mask wanted and not
  apply.res1           ssv_bn_apply                  a materialised residual
  apply.res2           ssv_bn_apply                  residual * rscale + rshift
  bwd.relu0            ssv_bn_train_bwd              no ReLU
  bwd.relu_y           ssv_bn_train_bwd              gate from the sign of y
  bwd.relu_mask        ssv_bn_train_bwd              gate from the byte mask: the same bits as from y
  bwd.relu_affine      ssv_bn_relu_bwd_affine        gate recomputed as x * scale + shift > 0
  bwd.dres             ssv_bn_train_bwd              dresidual given / NULL
  bwd.acc              ssv_bn_train_bwd              accumulate 0 on NaN-prefilled dgamma / dbeta, accumulate 1 on a seeded prior, both NULL - each on every backward form
  bwdp.one_level       ssv_bn_bwd_from_partials      <= 2048 groups; coef = [A, mean, B, D] and A * g + B * (x - mean) + D == dx
  bwdp.factor32        ssv_bn_bwd_from_partials      > 2048 groups with cdiv(groups, 32) <= cap
  bwdp.factor_cap      ssv_bn_bwd_from_partials      > 2048 groups with cdiv(groups, 32) > cap
  stem.even            ssv_bn_relu_maxpool_fwd       H, W even
  stem.odd             ssv_bn_relu_maxpool_fwd       9 x 11
  stem.narrow          ssv_bn_relu_maxpool_bwd       W == RT exactly
  stem.xmax            ssv_bn_relu_maxpool_bwd       pooled-resolution reduction (xmax given)
  stem.full_res        ssv_bn_relu_maxpool_bwd       the full-resolution walk (xmax NULL)
  stem.fallback        ssv_bn_relu_maxpool_bwd       xmax given but dropped: the pooled plan has more partial blocks than the full-resolution plan.  Reached
                                                     through rounding at LARGE M (C 256, N 449, 11 x 11: 1011 > 1007 blocks), not on tiny maps
  stem.refused         ssv_bn_relu_maxpool_bwd       RT > W returns an error status; nn.bn_relu_maxpool, run with a tape, records the BatchNorm + max-pool route and its backward is under bar (a)
  stem.stride          ssv_bn_relu_maxpool_fwd       more than 16384 * 256 float4 groups (86 x 112 x 112 x 64): second trip of the grid-stride loop
  pool.edges           ssv_maxpool3x3s2_fwd          H or W of 1, 2, odd, even; windows clipped on both sides
  pool.ties            ssv_maxpool3x3s2_fwd          ReLU'd input (ties at zero) and an input quantised to 8 levels: arg-max == ATen's
  pool.nonfinite       ssv_maxpool3x3s2_fwd          -inf rows and a few NaNs: y and arg-max as ATen's (forward only)
  pool.stride          ssv_maxpool3x3s2_bwd          work > 4096 * 256 items: max-pool 24 x 112 x 112 x 64, GAP 512 x 49 x 512, layouts 24 x 3 x 224 x 224
  gap.shapes           ssv_gap_fwd                   HW 1, 16, 49, 3136; N * C / 4 below, at and not a multiple of 256
  layout.c1            ssv_nchw_to_nhwc              C 1
  layout.c3            ssv_nchw_to_nhwc              C 3
  layout.c64           ssv_nhwc_to_nchw              C 64
  pad.grow             ssv_pad_channels              3 -> 4 and 3 -> 24
  pad.shrink           ssv_pad_channels              4 -> 3 with accumulate 0 / 1
  pad.refused          ssv_pad_channels              cin == cout returns an error status
  group.g1             ssv_group_expand              groups 1
  group.g2             ssv_group_expand              groups 2
  group.g32            ssv_group_extract             groups 32 (Cg 4, K 128, 3 x 3)
  group.cg1            ssv_group_extract             Cg 1 (depthwise)
  ftrans.rs1           ssv_filter_transpose          K 48, C 132 (not multiples of 32), R * S 1
  ftrans.rs9           ssv_filter_transpose          R * S 9
  ftrans.rs49          ssv_filter_transpose          R * S 49

Measured on an MI355X (profiles/bn_pool_kernels_report.json): see FACTOR / FLOOR below and DESIGN.md section 2.
"""
import json
import math
import os
import re
import subprocess
import zlib

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GUARD = 1024                                                             # floats of NaN behind every output
WS_GUARD = 4096                                                          # ... and behind every workspace
TAU = 2.0 ** -14                                                         # (b'): no pre-activation of a self-gated case closer to zero than this
EPS, MOMENTUM = 1e-5, 0.1
# one pair per family, set by the rule of the docstring from the MI355X run committed as profiles/bn_pool_kernels_report.json.  Measured worst ratios:
# bn-forward 2.62 (invstd at C 4, M 3000: 256 row lanes merged serially through LDS; y 2.56 there), bn-backward 2.30 (dgamma of the same case),
# reduction 1.12 (ssv_gap_fwd at HW 49, 512 x 512; HW 3136 sat at 9.64 under one serial sum per lane, which is why gap_fwd_k sums in runs of 64: 0.83).
FACTOR = {"bn-forward": 4.0, "bn-backward": 4.0, "reduction": 2.0}
# the final rounding of an fp32 result (2^-24 relative), twice where a prior is added: the resolution of the comparison, for every family
FLOOR = {"bn-forward": 2 * U, "bn-backward": 2 * U, "reduction": 2 * U}
COND = 1e-3                                                              # (b): ref32 further than this from ref64 measures nothing
REPORT = {}                                                              # case id -> tensor -> figures (SSV_BNPOOL_REPORT)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-supervised-vision_amd", "csrc")

FAMILY = {}
for _fam, _names in (("bn-forward", "y mean invstd scale shift running_mean running_var stem_out nn_out fwd_y fwd_mean fwd_invstd"),
                     ("bn-backward", "dx dres dgamma dbeta aff_dx aff_dgamma aff_dbeta coef dx_coef pool_dx stem_dy stem_dgamma stem_dbeta stem_dy_x stem_dgamma_x stem_dbeta_x nn_dy nn_dgamma nn_dbeta"),
                     ("reduction", "colsum gap_y gap_dx"),
                     ("exact", "mask pool_y pool_am nhwc nchw pad wd wg wt")):
    FAMILY.update({n: _fam for n in _names.split()})
# (e): the pooled-resolution reduction of the stem backward against the full-resolution walk
PAIRS = {"stem_dy_x": "stem_dy", "stem_dgamma_x": "stem_dgamma", "stem_dbeta_x": "stem_dbeta",
         "fwd_y": "y", "fwd_mean": "mean", "fwd_invstd": "invstd"}              # ... and ssv_bn_train_fwd against ssv_bn_train_fwd_partials on its own partition


def _s(x):
    """a scalar as the C ABI's float argument carries it"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _fmt(v):
    if isinstance(v, bool):
        return "y" if v else "n"
    if isinstance(v, (tuple, list)):
        return "x".join(_fmt(a) for a in v)
    return f"{v:g}" if isinstance(v, float) else str(v)


class Case:
    def __init__(self, kind, labels, **p):
        self.kind, self.labels, self.p = kind, tuple(labels.split()), p
        self.id = kind + "".join(f"-{k}{_fmt(v)}" for k, v in p.items())

    def __getitem__(self, k):
        return self.p.get(k)

    def gen(self):
        return torch.Generator().manual_seed(zlib.crc32(self.id.encode()))


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _t(inp, dt, *names):
    return [inp[n].detach().to(dt).clone() for n in names]


def cdiv(a, b):
    return -(-a // b)


# ====================================================================================================================== the plan, restated
def bn_plan(m, c):
    """bn_plan of bn.hip: float4 groups per row, channel groups / row lanes of a 256-thread block, y-blocks, rows per block, blocks"""
    c4 = c // 4
    ct = min(c4, 256)
    rt = 256 // ct
    rpb = max(cdiv(m, 1024), 4 * rt)
    return {"C4": c4, "CT": ct, "RT": rt, "GY": cdiv(c4, ct), "rpb": rpb, "nblk": cdiv(m, rpb)}


def apply_grid(p, m):
    """apply_grid of bn.hip: the element-wise passes get about 1024 workgroups in all"""
    rpb = max(cdiv(m, max(1024 // p["GY"], 1)), 4 * p["RT"])
    return {"rpb": rpb, "nblk": cdiv(m, rpb)}


def ws_floats(m, c):
    return 2 * bn_plan(m, c)["nblk"] * c + 2 * c


def lane_rows(m, rpb, rt):
    """rows each lane of each block walks (the unrolled loop takes 4 per trip, the tail loop the rest)"""
    out = set()
    for rows in {min(rpb, m), m - (cdiv(m, rpb) - 1) * rpb}:
        out |= {cdiv(rows - lane, rt) for lane in range(min(rt, rows))}
    return out


def merge_plan(groups, cap):
    """launch_finalize / ssv_bn_bwd_from_partials: None for the one-level merge, else (factor, coarse groups)"""
    if groups <= 2048:
        return None
    factor = cdiv(groups, cap) if cap > 0 and cdiv(groups, 32) > cap else 32
    return factor, cdiv(groups, factor)


# ====================================================================================================================== inputs and references
# Every kind has inputs(case) -> {name: CPU tensor} and ref(case, inputs, dtype) -> {name: tensor}: plain torch, run in float64 and in float32.
# Nothing here touches the library or the GPU.
def _stats64(x64):
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    return mean, var, 1.0 / (var + _s(EPS)).sqrt()


def _nudge(x, pre, slope):
    """(b'): x with every fp64 pre-activation inside TAU moved to 4 TAU on its own side; pre(x64) -> a64, slope(x64) -> da / dx"""
    for _ in range(2):
        x64 = x.double()
        a = pre(x64)
        near = a.abs() < TAU
        if not bool(near.any()):
            break
        target = torch.where(a >= 0, 4 * TAU, -4 * TAU)
        x = (x64 + torch.where(near, (target - a) / slope(x64), torch.zeros((), dtype=torch.float64))).float()
    return x


def _pack_mask(gate):
    """one byte per float4: bit e = element e positive (bn_apply_k)"""
    b = gate.reshape(-1, 4).to(torch.uint8)
    return b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)


def _bn_base(c, g):
    m, ch = c["M"], c["C"]
    mu, sd = float(c["mean"] or 0.0), float(c["std"] or 1.0)
    inp = {"x": _rn(g, m, ch, scale=sd) + mu + _rn(g, ch, scale=0.5 * sd), "gamma": torch.rand(ch, generator=g) + 0.5, "beta": _rn(g, ch, scale=0.3),
           "rm0": _rn(g, ch, scale=0.1), "rv0": torch.rand(ch, generator=g) + 1.0}
    if c["res"]:
        inp["res"] = _rn(g, m, ch)
    if c["relu"]:
        def pre(x64):
            mean, _, invstd = _stats64(x64)
            a = (x64 - mean) * (invstd * inp["gamma"].double()) + inp["beta"].double()
            return a + inp["res"].double() if c["res"] else a
        inp["x"] = _nudge(inp["x"], pre, lambda x64: _stats64(x64)[2] * inp["gamma"].double())
    return inp


def _bn_fwd_lines(c, inp, dt, out):
    x, gamma, beta, rm0, rv0 = _t(inp, dt, "x", "gamma", "beta", "rm0", "rv0")
    m = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / (var + _s(EPS)).sqrt()
    scale = gamma * invstd
    shift = beta - mean * scale
    a = x * scale + shift
    if c["res"]:
        a = a + inp["res"].to(dt)
    out.update({"y": a.clamp_min(0.0) if c["relu"] else a, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift})
    if c["relu"]:
        out["mask"] = _pack_mask(a > 0)
    if c["momentum"] is not None:
        mom = _s(c["momentum"])
        unbiased = var * (m / (m - 1.0)) if m > 1 else var
        out.update({"running_mean": (1.0 - mom) * rm0 + mom * mean, "running_var": (1.0 - mom) * rv0 + mom * unbiased})
    return a


def _bn_bwd_lines(dt, x, g, gamma, mean, invstd):
    m = x.shape[0]
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    return gamma * invstd * (g - dbeta / m - xhat * (dgamma / m)), dgamma, dbeta


# ---- ssv_bn_train_fwd, ssv_bn_train_bwd, ssv_bn_relu_bwd_affine, ssv_colsum --------------------------------------------------------------------------
def _bn_in(c):
    g = c.gen()
    inp = _bn_base(c, g)
    m, ch = c["M"], c["C"]
    x64 = inp["x"].double()
    mean, _, invstd = _stats64(x64)
    # the backward's inputs are data: the fp64 statistics, the fp64 forward's y and its gate, all rounded to fp32
    inp["mean_in"], inp["invstd_in"] = mean.float(), invstd.float()
    inp["scale_in"] = (inp["gamma"].double() * invstd).float()
    inp["shift_in"] = (inp["beta"].double() - mean * inp["scale_in"].double()).float()
    a = x64 * inp["scale_in"].double() + inp["shift_in"].double()
    if c["relu"]:
        inp["gate_aff"] = a > 0                                          # the sign of the kernel's fmaf
        if c["res"]:
            a = a + inp["res"].double()
        inp["y_in"] = a.clamp_min(0.0).float()
        inp["gate"] = inp["y_in"] > 0
    inp.update({"dy": _rn(g, m, ch), "dg0": _rn(g, ch), "db0": _rn(g, ch), "cs0": _rn(g, ch)})
    return inp


def _bn_ref(c, inp, dt):
    out = {}
    _bn_fwd_lines(c, inp, dt, out)
    del out["scale"], out["shift"]                                       # they live in ssv_bn_train_fwd's workspace
    x, gamma, dy, mean, invstd, dg0, db0, cs0 = _t(inp, dt, "x", "gamma", "dy", "mean_in", "invstd_in", "dg0", "db0", "cs0")
    acc = c["acc"] == "acc"
    g = dy * inp["gate"].to(dt) if c["relu"] else dy
    dx, dgamma, dbeta = _bn_bwd_lines(dt, x, g, gamma, mean, invstd)
    out["dx"] = dx
    if c["dres"]:
        out["dres"] = g
    if c["acc"] != "null":
        out.update({"dgamma": dgamma + dg0 if acc else dgamma, "dbeta": dbeta + db0 if acc else dbeta})
    if c["relu"] and not c["res"]:
        dx, dgamma, dbeta = _bn_bwd_lines(dt, x, dy * inp["gate_aff"].to(dt), gamma, mean, invstd)
        out.update({"aff_dx": dx, "aff_dgamma": dgamma + dg0 if acc else dgamma, "aff_dbeta": dbeta + db0 if acc else dbeta})
    out["colsum"] = x.sum(0) + cs0 if acc else x.sum(0)
    return out


def _bn_gate_check(c, inp):
    """(b'): fp64 and fp32 pre-activations of a case whose kernel decides its own gate, else None"""
    if not c["relu"] or c.kind not in ("bn", "part"):
        return None
    return _bn_fwd_lines(c, inp, torch.float64, {}), _bn_fwd_lines(c, inp, torch.float32, {})


# ---- ssv_bn_train_fwd_partials, ssv_bn_stats_finalize -------------------------------------------------------------------------------------------------
def _group_sums(rpg, *cols):
    """per group of rpg rows (the last ragged): [sum of every column tensor]"""
    m = cols[0].shape[0]
    full = m // rpg
    outs = []
    for t in cols:
        parts = [t[:full * rpg].view(full, rpg, -1).sum(1)] if full else []
        if m > full * rpg:
            parts.append(t[full * rpg:].sum(0, keepdim=True))
        outs.append(torch.cat(parts, 0))
    return outs


def _part_in(c):
    g = c.gen()
    inp = _bn_base(c, g)
    rpg, m = c["rpg"], c["M"]
    x64 = inp["x"].double()
    (s1,) = _group_sums(rpg, x64)
    n = torch.full((s1.shape[0], 1), float(rpg), dtype=torch.float64)
    n[-1] = m - (s1.shape[0] - 1) * rpg
    pmean = s1 / n
    (pm2,) = _group_sums(rpg, (x64 - pmean.repeat_interleave(rpg, 0)[:m]) ** 2)
    inp["pmean"], inp["pm2"] = pmean.float(), pm2.float()               # what a producer's epilogue hands over: (mean_b, M2_b) per group, in fp32
    return inp


def _part_ref(c, inp, dt):
    out = {}
    _bn_fwd_lines(c, inp, dt, out)
    if c["own"]:
        out.update({"fwd_y": out["y"], "fwd_mean": out["mean"], "fwd_invstd": out["invstd"]})
    return out


# ---- ssv_bn_apply --------------------------------------------------------------------------------------------------------------------------------------
def _apply_in(c):
    g = c.gen()
    m, ch = c["M"], c["C"]
    inp = {"x": _rn(g, m, ch, scale=2.0) + 0.3, "scale": (torch.rand(ch, generator=g) + 0.5) * torch.where(torch.rand(ch, generator=g) < 0.2, -1.0, 1.0),
           "shift": _rn(g, ch, scale=0.7)}
    if c["res"]:
        inp["res"] = _rn(g, m, ch)
    if c["res"] == 2:
        inp["rscale"], inp["rshift"] = torch.rand(ch, generator=g) + 0.5, _rn(g, ch, scale=0.4)
    if c["relu"] and c["res"]:                                          # the residual add rounds a second time: keep the sum away from zero
        inp["x"] = _nudge(inp["x"], lambda x64: _apply_lines(c, dict(inp, x=x64), torch.float64), lambda x64: inp["scale"].double())
    return inp


def _apply_lines(c, inp, dt):
    x, scale, shift = _t(inp, dt, "x", "scale", "shift")
    v = x * scale + shift
    if c["res"] == 1:
        v = v + inp["res"].to(dt)
    if c["res"] == 2:
        v = v + (inp["res"].to(dt) * inp["rscale"].to(dt) + inp["rshift"].to(dt))
    return v


def _apply_ref(c, inp, dt):
    v = _apply_lines(c, inp, dt)
    if not c["relu"]:
        return {"y": v}
    gate = _apply_lines(c, inp, torch.float64) > 0
    out = {"y": v * gate.to(dt)}
    if c["mask"]:
        out["mask"] = _pack_mask(gate)
    return out


# ---- ssv_bn_bwd_from_partials, ssv_bn_bwd_coef -------------------------------------------------------------------------------------------------------
def _bwdp_in(c):
    g = c.gen()
    m, ch, rpg = c["M"], c["C"], c["rpg"]
    inp = {"x": _rn(g, m, ch) + _rn(g, ch, scale=0.5), "gamma": torch.rand(ch, generator=g) + 0.5, "dg0": _rn(g, ch), "db0": _rn(g, ch)}
    inp["g"] = _rn(g, m, ch) * (torch.rand(m, ch, generator=g) < 0.6)  # arrives ReLU-gated
    x64, g64 = inp["x"].double(), inp["g"].double()
    mean, _, invstd = _stats64(x64)
    inp["mean_in"], inp["invstd_in"] = mean.float(), invstd.float()
    xhat = (x64 - inp["mean_in"].double()) * inp["invstd_in"].double()
    psg, psgx = _group_sums(rpg, g64, g64 * xhat)
    inp["psum_g"], inp["psum_gx"] = psg.float(), psgx.float()          # what the gating convolution's epilogue hands over, in fp32
    return inp


def _bwdp_ref(c, inp, dt):
    x, g, gamma, mean, invstd, dg0, db0 = _t(inp, dt, "x", "g", "gamma", "mean_in", "invstd_in", "dg0", "db0")
    m = x.shape[0]
    dx, dgamma, dbeta = _bn_bwd_lines(dt, x, g, gamma, mean, invstd)
    gi = gamma * invstd
    coef = torch.stack((gi, mean, -gi * invstd * (dgamma / m), -gi * (dbeta / m)))
    acc = c["acc"] == "acc"
    return {"dx": dx, "dgamma": dgamma + dg0 if acc else dgamma, "dbeta": dbeta + db0 if acc else dbeta, "coef": coef,
            "dx_coef": coef[0] * g + coef[2] * (x - coef[1]) + coef[3]}


# ---- max-pool 3 x 3 / 2 / 1 in NHWC --------------------------------------------------------------------------------------------------------------------
def _pool_nhwc(x):
    """ATen's max_pool2d on the NCHW view: (pooled NHWC, window slot r * 3 + s of the arg-max as uint8 NHWC, flat arg-max indices NCHW)"""
    n, h, w, ch = x.shape
    y, idx = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 3, 2, 1, return_indices=True)
    ho, wo = y.shape[2], y.shape[3]
    ih, iw = idx // w, idx % w
    slot = (ih - (2 * torch.arange(ho).view(1, 1, ho, 1) - 1)) * 3 + (iw - (2 * torch.arange(wo).view(1, 1, 1, wo) - 1))
    return y.permute(0, 2, 3, 1).contiguous(), slot.to(torch.uint8).permute(0, 2, 3, 1).contiguous(), idx


def _slots_to_idx(am, h, w):
    """window slots (uint8 NHWC) -> flat arg-max indices NCHW"""
    n, ho, wo, ch = am.shape
    s = am.permute(0, 3, 1, 2).long()
    return (2 * torch.arange(ho).view(1, 1, ho, 1) - 1 + s // 3) * w + (2 * torch.arange(wo).view(1, 1, 1, wo) - 1 + s % 3)


def _scatter(dy, idx, h, w):
    """max-pool backward: dy (NHWC) scattered to the arg-max pixels, NHWC"""
    n, ho, wo, ch = dy.shape
    out = torch.zeros(n, ch, h * w, dtype=dy.dtype)
    out.scatter_add_(2, idx.reshape(n, ch, -1), dy.permute(0, 3, 1, 2).reshape(n, ch, -1))
    return out.view(n, ch, h, w).permute(0, 2, 3, 1).contiguous()


def _pool_in(c):
    g = c.gen()
    n, h, w, ch = c["shape"]
    x = _rn(g, n, h, w, ch)
    if c["mode"] == "relu":
        x = x.clamp_min(0.0)
    if c["mode"] == "quant":
        x = torch.randint(0, 8, (n, h, w, ch), generator=g).float() * 0.25 - 1.0
    if c["mode"] == "nonfinite":
        x[:, ::3] = float("-inf")                                        # whole rows, so some windows see nothing else
        x.view(-1)[torch.randint(0, x.numel(), (max(x.numel() // 50, 3),), generator=g)] = float("nan")
    return {"x": x, "dy": _rn(g, n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, ch)}


def _pool_ref(c, inp, dt):
    x, dy = _t(inp, dt, "x", "dy")
    n, h, w, ch = c["shape"]
    y, am, idx = _pool_nhwc(x)
    out = {"pool_y": y, "pool_am": am}
    if c["mode"] != "nonfinite":
        out["pool_dx"] = _scatter(dy, idx, h, w)
    return out


def _pool_terms(c, inp):
    """how many dy terms every input pixel collects"""
    n, h, w, ch = c["shape"]
    _, _, idx = _pool_nhwc(inp["x"])
    return _scatter(torch.ones_like(inp["dy"]), idx, h, w)


# ---- the fused stem: BatchNorm + ReLU + max-pool -------------------------------------------------------------------------------------------------------
def _stem_in(c):
    g = c.gen()
    n, h, w, ch = c["shape"]
    inp = {"y": _rn(g, n, h, w, ch, scale=1.5) + 0.3 + _rn(g, ch, scale=0.5), "gamma": torch.rand(ch, generator=g) + 0.5, "beta": _rn(g, ch, scale=0.3)}
    if c["refused"]:                                                     # (b'): nn.bn_relu_maxpool computes the statistics itself, so the gate is the kernel's own
        def pre(y64):
            mean, _, invstd = _stats64(y64)
            return (y64 - mean) * (invstd * inp["gamma"].double()) + inp["beta"].double()
        inp["y"] = _nudge(inp["y"].view(-1, ch), pre, lambda y64: _stats64(y64)[2] * inp["gamma"].double()).view(n, h, w, ch)
    y64 = inp["y"].double().view(-1, ch)
    mean, _, invstd = _stats64(y64)
    inp["mean_in"], inp["invstd_in"] = mean.float(), invstd.float()
    inp["scale_in"] = (inp["gamma"].double() * invstd).float()
    inp["shift_in"] = (inp["beta"].double() - mean * inp["scale_in"].double()).float()
    if c["fwd_only"]:
        return inp
    a = (y64 * inp["scale_in"].double() + inp["shift_in"].double()).view(n, h, w, ch)
    inp["gate"] = a > 0
    _, am, idx = _pool_nhwc(a.clamp_min_(0.0))
    del a
    inp["am_in"] = am                                                    # (c): the backward's arg-max and xmax are data - the fp64 forward's
    inp["xmax_in"] = inp["y"].permute(0, 3, 1, 2).reshape(n, ch, -1).gather(2, idx.view(n, ch, -1)).view(n, ch, am.shape[1], am.shape[2]).permute(0, 2, 3, 1).contiguous()
    inp.update({"dpool": _rn(g, *am.shape), "dg0": _rn(g, ch), "db0": _rn(g, ch)})
    if c["refused"]:                                                     # nn.bn_relu_maxpool starts from the convolution's statistics partials
        rows = n * h * w
        (s1,) = _group_sums(64, y64)
        cnt = torch.full((s1.shape[0], 1), 64.0, dtype=torch.float64)
        cnt[-1] = rows - (s1.shape[0] - 1) * 64
        pmean = s1 / cnt
        (pm2,) = _group_sums(64, (y64 - pmean.repeat_interleave(64, 0)[:rows]) ** 2)
        inp["pmean"], inp["pm2"] = pmean.float(), pm2.float()
    return inp


def _stem_own_lines(c, inp, dt):
    """the unfused route of nn.bn_relu_maxpool, statistics and arg-max its own: (pre-activation, pooled, flat arg-max indices)"""
    n, h, w, ch = c["shape"]
    y, gamma, beta = _t(inp, dt, "y", "gamma", "beta")
    y = y.view(-1, ch)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    invstd = 1.0 / (var + _s(EPS)).sqrt()
    scale = gamma * invstd
    a = (y * scale + (beta - mean * scale)).view(n, h, w, ch)
    pooled, _, idx = _pool_nhwc(a.clamp_min(0.0))
    return a, pooled, idx, mean, invstd


def _stem_ref(c, inp, dt):
    n, h, w, ch = c["shape"]
    if c["refused"]:
        a, pooled, idx, mean, invstd = _stem_own_lines(c, inp, dt)
        y, gamma, dpool = _t(inp, dt, "y", "gamma", "dpool")
        g = _scatter(dpool, idx, h, w) * (a > 0).to(dt)
        dy, dgamma, dbeta = _bn_bwd_lines(dt, y.view(-1, ch), g.view(-1, ch), gamma, mean, invstd)
        return {"nn_out": pooled, "nn_dy": dy.view(n, h, w, ch), "nn_dgamma": dgamma, "nn_dbeta": dbeta}
    y, scale, shift = _t(inp, dt, "y", "scale_in", "shift_in")
    r = (y * scale + shift).clamp_min_(0.0)
    pooled = F.max_pool2d(r.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    del r
    out = {"stem_out": pooled}
    if c["fwd_only"]:
        return out
    gamma, mean, invstd, dpool, dg0, db0 = _t(inp, dt, "gamma", "mean_in", "invstd_in", "dpool", "dg0", "db0")
    g = _scatter(dpool, _slots_to_idx(inp["am_in"], h, w), h, w) * inp["gate"].to(dt)
    dy, dgamma, dbeta = _bn_bwd_lines(dt, y.view(-1, ch), g.view(-1, ch), gamma, mean, invstd)
    acc = c["acc"] == "acc"
    out.update({"stem_dy": dy.view(n, h, w, ch), "stem_dgamma": dgamma + dg0 if acc else dgamma, "stem_dbeta": dbeta + db0 if acc else dbeta})
    for k in ("stem_dy", "stem_dgamma", "stem_dbeta"):
        out[k + "_x"] = out[k]
    return out


# ---- global average pool -------------------------------------------------------------------------------------------------------------------------------
def _gap_in(c):
    g = c.gen()
    n, hw, ch = c["shape"]
    return {"x": _rn(g, n, hw, ch) + 0.4, "dy": _rn(g, n, ch)}


def _gap_ref(c, inp, dt):
    x, dy = _t(inp, dt, "x", "dy")
    hw = c["shape"][1]
    return {"gap_y": x.sum(1) / hw, "gap_dx": (dy / hw)[:, None, :].expand(-1, hw, -1).contiguous()}


# ---- layouts, channel padding, grouped filters, filter transpose: permutations, exact ---------------------------------------------------------------------
def _layout_in(c):
    g = c.gen()
    n, ch, h, w = c["shape"]
    return {"nchw_in": _rn(g, n, ch, h, w), "nhwc_in": _rn(g, n, h, w, ch)}


def _layout_ref(c, inp, dt):
    a, b = _t(inp, dt, "nchw_in", "nhwc_in")
    return {"nhwc": a.permute(0, 2, 3, 1).contiguous(), "nchw": b.permute(0, 3, 1, 2).contiguous()}


def _pad_in(c):
    g = c.gen()
    return {"t": _rn(g, c["npix"], c["cin"]), "prior": _rn(g, c["npix"], c["cout"])}


def _pad_ref(c, inp, dt):
    t, prior = _t(inp, dt, "t", "prior")
    cin, cout = c["cin"], c["cout"]
    if cout > cin:
        return {"pad": F.pad(t, (0, cout - cin))}
    return {"pad": prior + t[:, :cout] if c["acc"] else t[:, :cout].clone()}


def _group_in(c):
    g = c.gen()
    k, r, s, cg, groups = c["K"], c["R"], c["S"], c["Cg"], c["groups"]
    return {"w": _rn(g, k, r, s, cg), "dwd": _rn(g, k, r, s, cg * groups), "prior": _rn(g, k, r, s, cg)}


def _group_ref(c, inp, dt):
    w, dwd, prior = _t(inp, dt, "w", "dwd", "prior")
    k, cg, groups = c["K"], c["Cg"], c["groups"]
    kg = k // groups
    wd, wg = torch.zeros_like(dwd), torch.empty_like(w)
    for j in range(groups):                                             # networks/resnet.py's grouped convolution as a block-diagonal dense one
        wd[j * kg:(j + 1) * kg, :, :, j * cg:(j + 1) * cg] = w[j * kg:(j + 1) * kg]
        wg[j * kg:(j + 1) * kg] = dwd[j * kg:(j + 1) * kg, :, :, j * cg:(j + 1) * cg]
    return {"wd": wd, "wg": prior + wg if c["acc"] else wg}


def _ftrans_in(c):
    return {"w": _rn(c.gen(), c["K"], c["R"], c["S"], c["C"])}


def _ftrans_ref(c, inp, dt):
    (w,) = _t(inp, dt, "w")
    return {"wt": w.flip(1, 2).permute(3, 1, 2, 0).contiguous()}        # wt[c][R-1-r][S-1-s][k] = w[k][r][s][c]


# ====================================================================================================================== the case table
_BN = "ssv_bn_train_fwd ssv_bn_train_bwd ssv_bn_relu_bwd_affine ssv_bn_apply ssv_colsum"
KINDS = {
    # kind: (entry points reached, inputs, reference)
    "bn": (_BN, _bn_in, _bn_ref),
    "part": ("ssv_bn_train_fwd_partials ssv_bn_stats_finalize ssv_bn_apply", _part_in, _part_ref),
    "apply": ("ssv_bn_apply", _apply_in, _apply_ref),
    "bwdp": ("ssv_bn_bwd_from_partials ssv_bn_bwd_coef", _bwdp_in, _bwdp_ref),
    "stem": ("ssv_bn_relu_maxpool_fwd ssv_bn_relu_maxpool_bwd ssv_bn_apply ssv_maxpool3x3s2_fwd ssv_maxpool3x3s2_bwd ssv_bn_train_bwd ssv_bn_train_fwd_partials", _stem_in, _stem_ref),
    "pool": ("ssv_maxpool3x3s2_fwd ssv_maxpool3x3s2_bwd", _pool_in, _pool_ref),
    "gap": ("ssv_gap_fwd ssv_gap_bwd", _gap_in, _gap_ref),
    "layout": ("ssv_nchw_to_nhwc ssv_nhwc_to_nchw", _layout_in, _layout_ref),
    "pad": ("ssv_pad_channels", _pad_in, _pad_ref),
    "group": ("ssv_group_expand ssv_group_extract", _group_in, _group_ref),
    "ftrans": ("ssv_filter_transpose", _ftrans_in, _ftrans_ref),
}

_RELU = "bwd.relu_y bwd.relu_mask bwd.relu_affine "
CASES = [
    # ---- BatchNorm forward + backward + column sum: (M, C), ReLU, residual, momentum (None: running statistics NULL), dresidual, accumulate mode
    Case("bn", "plan.min_rows stats.running bwd.acc " + _RELU, M=1800, C=64, relu=True, momentum=0.1, acc="ow"),
    Case("bn", "plan.min_rows stats.running bwd.relu0 bwd.dres bwd.acc", M=1800, C=64, relu=False, res=True, dres=True, momentum=1.0, acc="acc"),
    Case("bn", "plan.min_rows stats.running bwd.relu_y bwd.relu_mask bwd.dres bwd.acc", M=1800, C=64, relu=True, res=True, dres=True, momentum=None, acc="null"),
    Case("bn", "plan.min_rows bwd.acc " + _RELU, M=1800, C=64, relu=True, momentum=0.1, acc="null"),
    Case("bn", "plan.rpb_grows bwd.acc stats.running " + _RELU, M=200003, C=64, relu=True, momentum=0.1, acc="acc"),
    Case("bn", "plan.rpb_grows stats.offset bwd.relu0", M=200003, C=64, relu=False, momentum=0.1, acc="ow", mean=30.0, std=0.03),
    Case("bn", "plan.idle_lanes bwd.dres " + _RELU, M=4099, C=96, relu=True, momentum=0.1, acc="ow"),
    Case("bn", "plan.idle_lanes bwd.relu_y bwd.relu_mask bwd.dres", M=2999, C=132, relu=True, res=True, dres=True, momentum=0.1, acc="acc"),
    Case("bn", "plan.idle_lanes bwd.relu0", M=70000, C=132, relu=False, momentum=0.1, acc="ow", mean=5.0, std=0.5),
    Case("bn", "plan.c4 plan.unroll_tail bwd.relu0", M=5, C=4, relu=False, momentum=0.1, acc="ow"),
    Case("bn", "plan.c4 " + _RELU, M=3000, C=4, relu=True, momentum=0.1, acc="acc"),
    Case("bn", "plan.gy2 plan.unroll_tail " + _RELU, M=5000, C=2048, relu=True, momentum=0.1, acc="ow", tail=1, atail=2),
    Case("bn", "plan.gy2 bwd.relu0 bwd.dres", M=5000, C=2048, relu=False, res=True, dres=True, momentum=0.1, acc="acc"),
    Case("bn", "plan.gy_ragged " + _RELU, M=300, C=1028, relu=True, momentum=0.1, acc="ow"),
    Case("bn", "plan.gy_ragged bwd.relu0", M=4103, C=1028, relu=False, momentum=None, acc="null"),
    Case("bn", "plan.unroll_tail " + _RELU, M=6000, C=1024, relu=True, momentum=0.1, acc="ow", tail=2),
    Case("bn", "plan.unroll_tail bwd.relu0", M=7000, C=1024, relu=False, momentum=0.1, acc="ow", tail=3),
    Case("bn", "plan.unroll_tail " + _RELU, M=81920, C=64, relu=True, momentum=0.1, acc="ow", tail=1),
    Case("bn", "stats.m1 bwd.relu0", M=1, C=64, relu=False, momentum=0.1, acc="ow"),
    Case("bn", "stats.m1 stats.running bwd.relu0", M=1, C=132, relu=False, momentum=1.0, acc="acc"),
    # ---- BatchNorm from the producer's statistics partials: rows per group
    Case("part", "partials.one_level", M=1500, C=64, rpg=1, relu=True, momentum=0.1),
    Case("part", "partials.one_level", M=20011, C=64, rpg=64, relu=True, res=True, momentum=0.1),
    Case("part", "partials.one_level", M=20011, C=132, rpg=64, relu=False, momentum=None),
    Case("part", "partials.one_level", M=449 * 121, C=256, rpg=121, relu=False, momentum=1.0),
    Case("part", "partials.one_level partials.own_partition", M=70001, C=64, rpg=69, relu=True, momentum=0.1, own=True),
    Case("part", "partials.factor32", M=200000, C=64, rpg=64, relu=True, momentum=0.1),
    Case("part", "partials.factor32", M=140003, C=64, rpg=64, relu=False, momentum=0.1),
    Case("part", "partials.factor32", M=140003, C=64, rpg=64, relu=False, momentum=0.1, mean=30.0, std=0.03),
    Case("part", "partials.one_level", M=100003, C=64, rpg=64, relu=False, momentum=0.1, mean=30.0, std=0.03),
    Case("part", "partials.factor_cap", M=5000, C=8, rpg=1, relu=True, momentum=0.1),
    Case("part", "partials.factor_cap", M=4999, C=8, rpg=2, relu=False, momentum=0.1),
    # ---- ssv_bn_apply: all six instantiations, mask wanted and not
    *[Case("apply", f"apply.res{r}", M=1500, C=96, res=r, relu=relu, mask=mask) for r in (0, 1, 2) for relu, mask in ((False, False), (True, False), (True, True))],
    Case("apply", "apply.res2 plan.gy2", M=5000, C=2048, res=2, relu=True, mask=True),
    Case("apply", "apply.res0 plan.gy2", M=5000, C=2048, res=0, relu=True, mask=True),
    Case("apply", "apply.res1 plan.unroll_tail", M=7000, C=1024, res=1, relu=False, mask=False, tail=3),
    # ---- the second half of the BatchNorm backward behind a gated convolution
    Case("bwdp", "bwdp.one_level", M=1500, C=64, rpg=1, acc="ow"),
    Case("bwdp", "bwdp.one_level", M=20011, C=132, rpg=64, acc="acc"),
    Case("bwdp", "bwdp.one_level", M=20011, C=64, rpg=64, acc="null"),
    Case("bwdp", "bwdp.factor32", M=200000, C=64, rpg=64, acc="ow"),
    Case("bwdp", "bwdp.factor32", M=140003, C=64, rpg=64, acc="acc"),
    Case("bwdp", "bwdp.factor_cap", M=5000, C=8, rpg=1, acc="ow"),
    Case("bwdp", "bwdp.factor_cap", M=4999, C=8, rpg=2, acc="acc"),
    # ---- the fused stem: (N, H, W, C)
    Case("stem", "stem.even stem.narrow stem.xmax stem.full_res", shape=(3, 12, 16, 64), acc="ow"),
    Case("stem", "stem.even stem.xmax stem.full_res", shape=(2, 56, 56, 64), acc="acc"),
    Case("stem", "stem.odd stem.xmax stem.full_res", shape=(5, 9, 11, 128), acc="ow"),
    Case("stem", "stem.odd stem.xmax stem.full_res", shape=(2, 23, 17, 64), acc="null"),
    Case("stem", "stem.fallback", shape=(449, 11, 11, 256), acc="ow"),
    Case("stem", "stem.refused", shape=(4, 16, 8, 64), acc="ow", refused=True),
    Case("stem", "stem.stride", shape=(86, 112, 112, 64), fwd_only=True),
    # ---- max-pool
    *[Case("pool", "pool.edges", shape=(2, h, w, 8), mode="normal", why=why) for h, w, why in ((1, 1, "one"), (1, 7, "one"), (7, 1, "one"), (2, 2, "two"), (2, 5, "two"),
                                                                                                (3, 3, "odd"), (9, 11, "odd"), (12, 16, "even"), (5, 4, "mixed"))],
    Case("pool", "pool.ties", shape=(3, 13, 14, 64), mode="relu"),
    Case("pool", "pool.ties", shape=(3, 13, 14, 64), mode="quant"),
    Case("pool", "pool.nonfinite", shape=(2, 11, 12, 16), mode="nonfinite"),
    Case("pool", "pool.stride pool.ties", shape=(24, 112, 112, 64), mode="relu"),
    # ---- global average pool: (N, HW, C)
    Case("gap", "gap.shapes", shape=(3, 1, 64)),
    Case("gap", "gap.shapes", shape=(4, 16, 256)),
    Case("gap", "gap.shapes", shape=(5, 49, 132)),
    Case("gap", "gap.shapes", shape=(9, 49, 132)),
    Case("gap", "gap.shapes", shape=(2, 3136, 64)),
    Case("gap", "gap.shapes pool.stride", shape=(512, 49, 512)),
    # ---- layouts: (N, C, H, W)
    Case("layout", "layout.c1", shape=(3, 1, 10, 14)),
    Case("layout", "layout.c3", shape=(3, 3, 10, 14)),
    Case("layout", "layout.c64", shape=(2, 64, 7, 9)),
    Case("layout", "layout.c3 pool.stride", shape=(24, 3, 224, 224)),
    # ---- channel padding
    Case("pad", "pad.grow", npix=1001, cin=3, cout=4),
    Case("pad", "pad.grow", npix=64 * 49, cin=3, cout=24),
    Case("pad", "pad.shrink", npix=64 * 49, cin=4, cout=3, acc=False),
    Case("pad", "pad.shrink", npix=64 * 49, cin=4, cout=3, acc=True),
    Case("pad", "pad.refused", npix=10, cin=4, cout=4),
    # ---- grouped filters
    Case("group", "group.g1", K=16, R=3, S=3, Cg=8, groups=1, acc=False),
    Case("group", "group.g2", K=10, R=1, S=1, Cg=5, groups=2, acc=True),
    Case("group", "group.g32", K=128, R=3, S=3, Cg=4, groups=32, acc=False),
    Case("group", "group.g32", K=128, R=3, S=3, Cg=4, groups=32, acc=True),
    Case("group", "group.cg1", K=24, R=3, S=3, Cg=1, groups=12, acc=False),
    # ---- filter transpose
    Case("ftrans", "ftrans.rs1", K=48, R=1, S=1, C=132),
    Case("ftrans", "ftrans.rs9", K=48, R=3, S=3, C=132),
    Case("ftrans", "ftrans.rs49", K=48, R=7, S=7, C=132),
    Case("ftrans", "ftrans.rs9", K=64, R=3, S=3, C=64),
]


# ====================================================================================================================== GPU-free honesty tests
def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(\S+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def launching_entry_points():
    """extern "C" functions of bn.hip and pool.hip that return a status (ssv_bn_workspace_bytes is a size query: it launches nothing)"""
    out = set()
    for name in ("bn.hip", "pool.hip"):
        with open(os.path.join(CSRC, name)) as f:
            out |= set(re.findall(r'^extern "C" int (ssv_\w+)\(', f.read(), flags=re.M))
    return out


def test_case_table_names_every_entry_point():
    """GPU-free: the entry points named by CASES are exactly the status-returning extern "C" functions of bn.hip and pool.hip."""
    named = {e for c in CASES for e in KINDS[c.kind][0].split()}
    have = launching_entry_points()
    assert len(have) >= 21
    assert named == have, f"missing {sorted(have - named)}, stray {sorted(named - have)}"


def test_case_table_covers_every_documented_branch():
    """GPU-free: every branch label of the docstring has a case, every label of a case is documented, the documented entry point is one the case's
    kind reaches, ids are unique, every output name has a family, and the bounds respect their caps."""
    doc = documented_labels()
    assert len(doc) >= 50
    used = {b for c in CASES for b in c.labels}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    for label, entry in doc.items():
        assert any(label in c.labels and entry in KINDS[c.kind][0].split() for c in CASES), (label, entry)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(FAMILY.values()) - {"exact"} == set(FACTOR) == set(FLOOR) and len(FACTOR) == 3
    assert all(1.0 <= f <= 8.0 and math.log2(f).is_integer() for f in FACTOR.values())
    assert all(0.0 <= f <= 16 * U for f in FLOOR.values())


def _partial_merge(c):
    m, ch = c["M"], c["C"]
    groups = cdiv(m, c["rpg"])
    return groups, bn_plan(m, ch)["nblk"], merge_plan(groups, bn_plan(m, ch)["nblk"])


def _stem_plans(c):
    n, h, w, ch = c["shape"]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return bn_plan(n * h * w, ch), bn_plan(n * ho * wo, ch)


def _mc(c):
    return bn_plan(c["M"], c["C"]), c["M"], c["C"]


def _has_tail(rows, tail):
    return any(r > 4 and r % 4 == tail for r in rows) if tail else any(0 < r < 4 for r in rows)


def _tail_ok(c):
    """per grid: `tail` rows per lane (mod 4) in the statistics grid (bn_stats_k, bn_bwd_reduce_k, colsum) and `atail` (default: the same) in the
    apply grid (bn_apply_k, bn_bwd_apply_k); ssv_bn_apply launches the apply grid only"""
    p, m, _ = _mc(c)
    stats, apply = lane_rows(m, p["rpb"], p["RT"]), lane_rows(m, apply_grid(p, m)["rpb"], p["RT"])
    atail = c["tail"] if c["atail"] is None else c["atail"]
    return _has_tail(apply, atail) and (c.kind == "apply" or _has_tail(stats, c["tail"]))


# label -> the property a case carrying it must have, in terms of the restated plan
PROPERTY = {
    "plan.min_rows": lambda c: _mc(c)[0]["rpb"] == 4 * _mc(c)[0]["RT"] and _mc(c)[0]["nblk"] > 1,
    "plan.rpb_grows": lambda c: (_mc(c)[0]["rpb"], _mc(c)[0]["nblk"], c["M"] - 1020 * 196) == (196, 1021, 83) and _mc(c)[0]["rpb"] > 4 * _mc(c)[0]["RT"],
    "plan.idle_lanes": lambda c: 256 % _mc(c)[0]["CT"] != 0 and _mc(c)[0]["RT"] * _mc(c)[0]["CT"] < 256,
    "plan.c4": lambda c: (_mc(c)[0]["CT"], _mc(c)[0]["RT"]) == (1, 256) and (c["M"] < 256 or c["M"] > 1024),
    "plan.gy2": lambda c: _mc(c)[0]["GY"] == 2 and apply_grid(_mc(c)[0], c["M"])["rpb"] != _mc(c)[0]["rpb"] and apply_grid(_mc(c)[0], c["M"])["nblk"] != _mc(c)[0]["nblk"],
    "plan.gy_ragged": lambda c: _mc(c)[0]["GY"] == 2 and _mc(c)[0]["C4"] - _mc(c)[0]["CT"] == 1,
    "plan.unroll_tail": _tail_ok,
    "stats.offset": lambda c: c["mean"] / c["std"] >= 999 and not c["relu"],
    "stats.m1": lambda c: c["M"] == 1,
    "partials.one_level": lambda c: _partial_merge(c)[2] is None,
    "partials.factor32": lambda c: _partial_merge(c)[2] is not None and _partial_merge(c)[2][0] == 32 and cdiv(_partial_merge(c)[0], 32) <= _partial_merge(c)[1],
    "partials.factor_cap": lambda c: _partial_merge(c)[2] is not None and cdiv(_partial_merge(c)[0], 32) > _partial_merge(c)[1] and _partial_merge(c)[2][0] > 32
    and _partial_merge(c)[2][1] <= _partial_merge(c)[1],
    "stem.even": lambda c: c["shape"][1] % 2 == 0 and c["shape"][2] % 2 == 0,
    "stem.odd": lambda c: c["shape"][1] % 2 == 1 and c["shape"][2] % 2 == 1,
    "stem.narrow": lambda c: _stem_plans(c)[0]["RT"] == c["shape"][2],
    "stem.xmax": lambda c: _stem_plans(c)[1]["nblk"] <= _stem_plans(c)[0]["nblk"] and _stem_plans(c)[0]["RT"] <= c["shape"][2],
    "stem.full_res": lambda c: _stem_plans(c)[0]["RT"] <= c["shape"][2],
    "stem.fallback": lambda c: _stem_plans(c)[1]["nblk"] > _stem_plans(c)[0]["nblk"] and (_stem_plans(c)[0]["nblk"], _stem_plans(c)[1]["nblk"]) == (1007, 1011),
    "stem.refused": lambda c: _stem_plans(c)[0]["RT"] > c["shape"][2],
    "stem.stride": lambda c: c["shape"][0] * ((c["shape"][1] + 1) // 2) * ((c["shape"][2] + 1) // 2) * c["shape"][3] // 4 > 16384 * 256,
    "gap.shapes": lambda c: c["shape"][1] in (1, 16, 49, 3136),
    "pad.refused": lambda c: c["cin"] == c["cout"],
    "pad.grow": lambda c: c["cin"] == 3 and c["cout"] in (4, 24),
    "pad.shrink": lambda c: (c["cin"], c["cout"]) == (4, 3),
}
PROPERTY["bwdp.one_level"], PROPERTY["bwdp.factor32"], PROPERTY["bwdp.factor_cap"] = (PROPERTY[f"partials.{k}"] for k in ("one_level", "factor32", "factor_cap"))


def _stride_ok(c):
    if c.kind == "pool":
        n, h, w, ch = c["shape"]
        return n * ((h + 1) // 2) * ((w + 1) // 2) * ch // 4 > 4096 * 256
    if c.kind == "gap":
        return math.prod(c["shape"]) // 4 > 4096 * 256
    n, ch, h, w = c["shape"]
    return n * h * w > 4096 * 256


PROPERTY["pool.stride"] = _stride_ok
PROPERTY["partials.own_partition"] = lambda c: c["rpg"] == _mc(c)[0]["rpb"] > 4 * _mc(c)[0]["RT"] and c["M"] % c["rpg"] != 0
PROPERTY.update({f"layout.c{k}": (lambda c, k=k: c["shape"][1] == k) for k in (1, 3, 64)})
PROPERTY.update({"group.g1": lambda c: c["groups"] == 1, "group.g2": lambda c: c["groups"] == 2,
                 "group.g32": lambda c: (c["groups"], c["Cg"], c["K"], c["R"] * c["S"]) == (32, 4, 128, 9), "group.cg1": lambda c: c["Cg"] == 1 and c["groups"] > 1})
PROPERTY.update({f"ftrans.rs{k}": (lambda c, k=k: c["R"] * c["S"] == k) for k in (1, 9, 49)})
PROPERTY["pool.edges"] = lambda c: {"one": min(c["shape"][1:3]) == 1, "two": min(c["shape"][1:3]) == 2, "odd": c["shape"][1] % 2 == c["shape"][2] % 2 == 1 and min(c["shape"][1:3]) >= 3,
                                    "even": c["shape"][1] % 2 == c["shape"][2] % 2 == 0 and min(c["shape"][1:3]) >= 4, "mixed": c["shape"][1] % 2 != c["shape"][2] % 2}[c["why"]]
PROPERTY["pool.ties"] = lambda c: c["mode"] in ("relu", "quant")
PROPERTY["pool.nonfinite"] = lambda c: c["mode"] == "nonfinite"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_shapes_have_the_property_their_label_claims(case):
    """GPU-free: per label, the chosen shape really reaches the branch under the plan as bn.hip / pool.hip compute it today."""
    for b in case.labels:
        if b in PROPERTY and (b.split(".")[0] != "plan" or case.kind in ("bn", "apply")):
            assert PROPERTY[b](case), f"{case.id} does not have the property of {b}"


def test_collective_shape_properties():
    """GPU-free: what a label asks of its cases together."""
    by = lambda label: [c for c in CASES if label in c.labels]
    assert {c["tail"] for c in by("plan.unroll_tail") if c.kind == "bn"} >= {None, 1, 2, 3}                      # the statistics grid ...
    assert {c["tail"] if c["atail"] is None else c["atail"] for c in by("plan.unroll_tail")} >= {None, 1, 2, 3}      # ... and the apply grid
    modes = {"ow", "acc", "null"}                                       # bwd.acc: every backward form sees all three accumulate modes
    bn = [c for c in CASES if c.kind == "bn"]
    assert {c["acc"] for c in bn if not c["relu"]} == modes, "ssv_bn_train_bwd, relu 0"
    assert {c["acc"] for c in bn if c["relu"]} == modes, "ssv_bn_train_bwd, relu 1"
    assert {c["acc"] for c in bn if c["relu"] and not c["res"]} == modes, "ssv_bn_relu_bwd_affine"
    assert {c["acc"] for c in CASES if c.kind == "bwdp"} == modes, "ssv_bn_bwd_from_partials / ssv_bn_bwd_coef"
    assert {c["acc"] for c in CASES if c.kind == "stem" and not c["fwd_only"] and not c["refused"]} == modes, "ssv_bn_relu_maxpool_bwd"
    assert {c["why"] for c in by("pool.edges")} == {"one", "two", "odd", "even", "mixed"}
    assert {c["C"] for c in by("plan.idle_lanes")} >= {96, 132} and {bn_plan(1, ch)["RT"] for ch in (96, 132)} == {10, 7}
    assert {c["M"] < 256 for c in by("plan.c4")} == {True, False}
    assert {c["momentum"] for c in by("stats.running")} >= {None, 0.1, 1.0}
    assert {c["acc"] for c in by("bwd.acc")} >= {"ow", "acc", "null"} and {bool(c["dres"]) for c in by("bwd.dres")} == {True, False}
    assert {c["rpg"] for c in by("partials.one_level")} >= {1, 64} and any(c["M"] % c["rpg"] for c in by("partials.one_level"))
    assert any(c["M"] % c["rpg"] for c in by("partials.factor32")) and any(c["M"] == 200000 for c in by("partials.factor32"))
    assert any(c["M"] % c["rpg"] for c in by("bwdp.factor32")) and any(c["M"] % c["rpg"] for c in by("bwdp.factor_cap"))
    assert {(c["res"], c["relu"], c["mask"]) for c in CASES if c.kind == "apply"} >= {(r, a, b) for r in (0, 1, 2) for a, b in ((False, False), (True, False), (True, True))}
    edges = {c["shape"][1:3] for c in by("pool.edges")}
    assert {h for h, _ in edges} >= {1, 2, 9, 12} and {w for _, w in edges} >= {1, 2, 11, 16}
    assert {c["mode"] for c in by("pool.ties")} == {"relu", "quant"}
    assert {c.kind for c in by("pool.stride")} == {"pool", "gap", "layout"}
    quarter = sorted(c["shape"][0] * c["shape"][2] // 4 for c in by("gap.shapes"))
    assert {c["shape"][1] for c in by("gap.shapes")} == {1, 16, 49, 3136} and quarter[0] < 256 and 256 in quarter and any(q > 256 and q % 256 for q in quarter)
    assert {c["groups"] for c in CASES if c.kind == "group"} >= {1, 2, 32} and {c["acc"] for c in CASES if c.kind == "group"} == {True, False}
    assert all(c["K"] % 32 and c["C"] % 32 for c in CASES if c.kind == "ftrans" and c["K"] == 48) and {c["R"] * c["S"] for c in CASES if c.kind == "ftrans"} == {1, 9, 49}


def test_restated_plan_is_the_plan_of_bn_plan_h(tmp_path):
    """GPU-free: tests/bn_plan_main.cpp + csrc/bn_plan.h compiled as a host program with -fsanitize=address,undefined, run over every (M, C) of CASES, every
    stem shape at full and pooled resolution and every (groups, cap) the part and bwdp cases reach: bn_plan, apply_grid, ws_floats and merge_plan above (and
    the pooled extent _stem_plans uses) give the numbers the C++ gives, both workspace layouts end where the workspace ends, and no sanitizer report."""
    cxx = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/usr/bin/clang++", "/usr/bin/g++") if os.path.exists(p)), "c++")
    exe = tmp_path / "bn_plan_main"
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                          os.path.join(ROOT, "tests", "bn_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    mcs, merges, pools = set(), set(), set()
    for c in CASES:
        if c["M"] and c["C"]:
            mcs.add((c["M"], c["C"]))
        if c.kind in ("part", "bwdp"):
            groups, cap, _ = _partial_merge(c)
            merges.add((groups, cap))
        if c.kind == "stem":
            n, h, w, ch = c["shape"]
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            mcs |= {(n * h * w, ch), (n * ho * wo, ch)}
            pools.add((h, w, ho, wo))
    assert len(mcs) >= 30 and len(pools) >= 7 and {merge_plan(*m) is None for m in merges} == {True, False}
    mcs, merges, pools = sorted(mcs), sorted(merges), sorted(pools)
    want = []
    for m, ch in mcs:
        p, g = bn_plan(m, ch), apply_grid(bn_plan(m, ch), m)
        want.append(f"plan {m} {ch} -> {p['C4']} {p['CT']} {p['RT']} {p['GY']} {p['rpb']} {p['nblk']} | {g['rpb']} {g['nblk']} | {ws_floats(m, ch)}")
    for groups, cap in merges:
        factor, ncoarse = merge_plan(groups, cap) or (0, groups)
        want.append(f"merge {groups} {cap} -> {factor} {ncoarse}")
    want += [f"pool {h} {w} -> {ho} {wo}" for h, w, ho, wo in pools]
    want.append(f"bn plans: {len(mcs)} plans, {len(merges)} merges")
    queries = tmp_path / "queries.txt"
    queries.write_text("".join(f"plan {m} {ch}\n" for m, ch in mcs) + "".join(f"merge {g} {cap}\n" for g, cap in merges) + "".join(f"pool {h} {w}\n" for h, w, _, _ in pools))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([str(exe), str(queries)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-4000:]
    got = run.stdout.splitlines()
    assert len(got) == len(want)
    for g, w_ in zip(got, want):
        assert g == w_, f"bn_plan.h says '{g}', the restatement in this file '{w_}'"


def _err(x, ref64):
    d = x.detach().double().cpu() - ref64
    return float(d.norm() / ref64.norm().clamp_min(1e-300)), float(d.abs().max() / ref64.abs().max().clamp_min(1e-300))


def _same(a, b):
    """bit-identical, a NaN equal to a NaN"""
    if not a.is_floating_point():
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


ZERO_OK = {"stats.m1": ("dx", "dgamma", "running_var")}                           # results a label declares exactly zero


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_is_well_conditioned(case):
    """GPU-free, conditions (b) and (b'): the fp64 reference is finite and not identically zero, the fp32 evaluation of the same lines is within 1e-3
    of it (e and m) and bit-identical for the family `exact`; no gate of a self-gated case is decided differently by fp32 and fp64."""
    _, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    assert set(r64) == set(r32) and set(r64) <= set(FAMILY)
    nonfinite = "pool.nonfinite" in case.labels
    for name, t in r64.items():
        if FAMILY[name] == "exact":
            assert _same(t.to(r32[name].dtype), r32[name]), f"{name}: the fp64 and fp32 references of an exact output differ"
            continue
        assert t.dtype == torch.float64 and r32[name].dtype == torch.float32, name
        assert nonfinite or (torch.isfinite(t).all() and torch.isfinite(r32[name]).all()), name
        zero_ok = any(name in ZERO_OK.get(b, ()) for b in case.labels)
        assert zero_ok or float(t.abs().max()) > 0, f"{name}: the reference is identically zero"
        e, m = _err(r32[name], t)
        print(f"{case.id} {name}: e(ref32) {e:.3e} m(ref32) {m:.3e}")
        assert e <= COND and m <= COND, f"{name}: ref32 is {e:.2e} / {m:.2e} from ref64 - the case measures nothing"
    gates = _bn_gate_check(case, inp)
    if case.kind == "apply" and case["relu"] and case["res"]:          # without a residual the gate is the sign of one fmaf: nothing to condition
        gates = _apply_lines(case, inp, torch.float64), _apply_lines(case, inp, torch.float32)
    if case["refused"]:
        own64, own32 = _stem_own_lines(case, inp, torch.float64), _stem_own_lines(case, inp, torch.float32)
        gates = own64[0], own32[0]
        assert torch.equal(own64[2], own32[2]), "fp32 and fp64 pick different arg-max pixels: the backward of this case measures nothing"
    if gates is not None:
        a64, a32 = gates
        flips = int(((a64 > 0) != (a32 > 0)).sum())
        print(f"{case.id}: min|a64| {float(a64.abs().min()):.3e} max|a32 - a64| {float((a32.double() - a64).abs().max()):.3e} gate flips {flips}")
        assert flips == 0
        assert float(a64.abs().min()) >= TAU, "an element is still inside TAU after two passes"
        assert float((a32.double() - a64).abs().max()) <= TAU / 4
    if case.kind == "pool" and not nonfinite:
        terms = _pool_terms(case, inp)
        assert float(terms.max()) <= 4 and (case["mode"] == "normal" or float(terms.max()) >= 2)


# ====================================================================================================================== GPU side
def _lib():
    from ssv_amd import _lib as L
    return L


def _ratio(got, ref, floor):
    if got <= floor:
        return 0.0
    return (got - floor) / ref if ref > 0 else float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib().load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_BNPOOL_REPORT")
    if path:
        fams = {f: {"FACTOR": FACTOR[f], "FLOOR": FLOOR[f], "worst_e_ratio": 0.0, "worst_m_ratio": 0.0, "worst_e_case": "", "worst_m_case": ""} for f in FACTOR}
        for cid, tensors in REPORT.items():
            for name, r in tensors.items():
                f = fams[FAMILY[name.split(" ")[0]]]
                for k in ("e", "m"):
                    ratio = _ratio(r[f"{k}_got"], r[f"{k}_ref32"], f["FLOOR"])
                    if ratio > f[f"worst_{k}_ratio"]:
                        f[f"worst_{k}_ratio"], f[f"worst_{k}_case"] = ratio, f"{cid} {name}"
        with open(path, "w") as fh:
            json.dump({"families": fams, "cases": REPORT}, fh, indent=1, sort_keys=True)


class Ctx:
    """The device side of one run of one case: uploaded inputs (kept to prove them untouched), guarded outputs, stated identities."""

    def __init__(self, dev):
        self.dev, self.ins, self.bufs, self.same = dev, [], [], []

    def up(self, name, t):
        """an input, 16-byte aligned, with a row (at least GUARD elements) of slack behind it: a kernel that over-reads by a row fails its case, it does not fault"""
        buf = torch.zeros((t.numel() + max(GUARD, t.shape[-1] if t.dim() else 0),), dtype=t.dtype, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        d = buf[:t.numel()].view(t.shape)
        d.copy_(t)
        self.ins.append((name, d, d.clone()))
        return d

    def out(self, name, shape, prior=None, nan_ok=False, guard=GUARD):
        """a 16-byte aligned view into a NaN-prefilled buffer: the payload is rounded up to a multiple of 4 floats before the guard"""
        n = math.prod(shape)
        buf = torch.full(((n + 3) // 4 * 4 + guard,), float("nan"), device=self.dev)
        assert buf.data_ptr() % 16 == 0
        if prior is not None:
            buf[:n].copy_(prior.reshape(-1))
        self.bufs.append((name, buf, n, nan_ok))
        return buf[:n].view(shape)

    def ws(self, name, nbytes):
        """a guarded workspace of the size the library asks for: (tensor, bytes)"""
        nbytes = int(nbytes)
        assert nbytes % 4 == 0
        return self.out(name, (nbytes // 4,), nan_ok=True, guard=WS_GUARD), nbytes

    def bytes(self, name, n):
        """a guarded byte output (ReLU mask, arg-max slots): 1024 sentinels behind it"""
        buf = torch.full(((n + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device=self.dev)
        buf[:n] = 0xEE
        self.bufs.append((name, buf, n, True))
        return buf[:n]

    def ints(self, name, values, dtype):
        """a guarded integer output: 64 sentinels behind it"""
        buf = torch.full((len(values) + 64,), -77, dtype=dtype, device=self.dev)
        buf[:len(values)] = torch.tensor(values, dtype=dtype)
        self.bufs.append((name, buf, len(values), False))
        return buf[:len(values)]

    def verify(self, what):
        torch.cuda.synchronize()
        for name, d, keep in self.ins:
            assert _same(d, keep), f"{what}: input {name} was modified"
        for name, buf, n, nan_ok in self.bufs:
            if buf.is_floating_point():
                assert nan_ok or not torch.isnan(buf[:n]).any(), f"{what} {name}: {int(torch.isnan(buf[:n]).sum())} elements never written (or NaN)"
                assert torch.isnan(buf[n:]).all(), f"{what} {name}: wrote past its end"
            elif buf.dtype == torch.uint8:
                assert (buf[n:] == 0xA5).all(), f"{what} {name}: wrote past its end"
            else:
                assert (buf[n:] == -77).all(), f"{what} {name}: wrote past its end"
        for name, a, b in self.same:
            assert _same(a, b), f"{what}: {name} not bit-identical (max |diff| {float((a.double() - b.double()).abs().max()):.3e})"


def _refused(fn, *args):
    """the call returns an error status (raised as SsvError by _lib.call): nothing was launched"""
    L = _lib()
    with pytest.raises(L.SsvError):
        L.call(fn, *args)


def _grads(ctx, c, inp, mode, ch, tag=""):
    """(dgamma, dbeta, accumulate) for an accumulate mode: ow = NaN-prefilled, overwrite; acc = seeded prior; zero = zero prior; null = both NULL"""
    if mode == "null":
        return None, None, 0
    pri = {"ow": (None, None), "acc": (inp["dg0"], inp["db0"]), "zero": (torch.zeros(ch), torch.zeros(ch))}[mode]
    return ctx.out("dgamma" + tag, (ch,), prior=pri[0]), ctx.out("dbeta" + tag, (ch,), prior=pri[1]), int(mode != "ow")


# ---- the runners: (case, inputs, ctx) -> {name: tensor}; exact statements are asserted inside ------------------------------------------------------------
def _bn_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    m, ch, relu = c["M"], c["C"], int(bool(c["relu"]))
    x, gamma, beta, dy = (ctx.up(nm, inp[nm]) for nm in ("x", "gamma", "beta", "dy"))
    res = ctx.up("res", inp["res"]) if c["res"] else None
    wsb = L.load().ssv_bn_workspace_bytes(m, ch)
    assert wsb == 4 * ws_floats(m, ch), "bn_plan as restated in this file is not the library's"
    mom = c["momentum"]

    def fwd():
        y, mean, invstd = ctx.out("y", (m, ch)), ctx.out("mean", (ch,)), ctx.out("invstd", (ch,))
        mask = ctx.bytes("mask", m * ch // 4) if relu else None
        rm = rv = nbt = None
        if mom is not None:
            rm, rv, nbt = ctx.out("running_mean", (ch,), prior=inp["rm0"]), ctx.out("running_var", (ch,), prior=inp["rv0"]), ctx.ints("nbt", [7], torch.int64)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_fwd", m, ch, P(x), P(gamma), P(beta), P(res), relu, EPS, 0.0 if mom is None else mom, P(rm), P(rv), P(nbt), P(y), P(mask),
               P(mean), P(invstd), P(ws), wsb, L.stream())
        if mom is not None:
            assert int(nbt) == 8, f"num_batches_tracked {int(nbt)} after one call on 7"
        out = {"y": y, "mean": mean, "invstd": invstd}
        if relu:
            out["mask"] = mask
        if mom is not None:
            out.update({"running_mean": rm, "running_var": rv})
        return out
    out, again = fwd(), fwd()
    ctx.same += [(f"ssv_bn_train_fwd, second call: {k}", out[k], again[k]) for k in out]
    if relu:
        nomask = ctx.out("y (no mask)", (m, ch))
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_fwd", m, ch, P(x), P(gamma), P(beta), P(res), relu, EPS, 0.0, None, None, None, P(nomask), None, P(ctx.out("mean", (ch,))),
               P(ctx.out("invstd", (ch,))), P(ws), wsb, L.stream())
        ctx.same.append(("ssv_bn_train_fwd without a mask: y", nomask, out["y"]))
    if m == 1:
        assert _same(out["mean"], x[0]), "M = 1: the mean is not the row itself"
        assert float((out["invstd"] * math.sqrt(_s(EPS)) - 1.0).abs().max()) < 4 * U, "M = 1: invstd is not 1 / sqrt(eps)"

    # ---- backward: its inputs are data
    mean_in, invstd_in = ctx.up("mean_in", inp["mean_in"]), ctx.up("invstd_in", inp["invstd_in"])
    y_in = ctx.up("y_in", inp["y_in"]) if relu else None
    mask_in = ctx.up("mask_in", _pack_mask(inp["gate"])) if relu else None

    def bwd(y_, mask_, mode, want_dres):
        dx = ctx.out("dx", (m, ch))
        dres = ctx.out("dres", (m, ch)) if want_dres else None
        dg, db, acc = _grads(ctx, c, inp, mode, ch)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_bwd", m, ch, P(dy), P(y_), P(mask_), P(x), P(gamma), P(mean_in), P(invstd_in), relu, P(dx), P(dres), P(dg), P(db), acc,
               P(ws), wsb, L.stream())
        return {k: v for k, v in (("dx", dx), ("dres", dres), ("dgamma", dg), ("dbeta", db)) if v is not None}
    got = bwd(y_in, None, c["acc"], bool(c["dres"]))
    again = bwd(y_in, None, c["acc"], bool(c["dres"]))
    ctx.same += [(f"ssv_bn_train_bwd, second call: {k}", got[k], again[k]) for k in got]
    zero, plain = bwd(y_in, None, "zero", False), bwd(y_in, None, "ow", not c["dres"])
    ctx.same += [(f"ssv_bn_train_bwd, accumulate on a zero prior vs overwrite: {k}", zero[k], plain[k]) for k in zero]
    ctx.same.append(("ssv_bn_train_bwd, dx with and without dresidual / dgamma", plain["dx"], got["dx"]))
    if relu:
        bymask = bwd(None, mask_in, c["acc"], bool(c["dres"]))
        ctx.same += [(f"ssv_bn_train_bwd from the byte mask vs from y: {k}", bymask[k], got[k]) for k in got]
    if m == 1:
        assert bool((got["dx"] == 0).all()), "M = 1: dx is not exactly zero"
    out.update(got)

    # ---- the gate recomputed from (scale, shift)
    if relu and not c["res"]:
        scale, shift = ctx.up("scale_in", inp["scale_in"]), ctx.up("shift_in", inp["shift_in"])

        def affine(mode):
            dx = ctx.out("aff_dx", (m, ch))
            dg, db, acc = _grads(ctx, c, inp, mode, ch, " (affine)")
            ws, _ = ctx.ws("workspace", wsb)
            L.call("ssv_bn_relu_bwd_affine", m, ch, P(dy), P(x), P(gamma), P(mean_in), P(invstd_in), P(scale), P(shift), P(dx), P(dg), P(db), acc, P(ws), wsb, L.stream())
            return dx, dg, db
        mode = "ow" if c["acc"] == "null" else c["acc"]
        aff = affine(mode)
        ya, ma = ctx.out("y (ssv_bn_apply)", (m, ch)), ctx.bytes("mask (ssv_bn_apply)", m * ch // 4)
        L.call("ssv_bn_apply", m, ch, P(x), P(scale), P(shift), None, None, None, 1, P(ya), P(ma), L.stream())
        dx = ctx.out("dx", (m, ch))
        dg, db, acc = _grads(ctx, c, inp, mode, ch)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_bwd", m, ch, P(dy), P(ya), None, P(x), P(gamma), P(mean_in), P(invstd_in), 1, P(dx), None, P(dg), P(db), acc, P(ws), wsb, L.stream())
        ctx.same += [(f"ssv_bn_relu_bwd_affine vs ssv_bn_train_bwd on the y of ssv_bn_apply: {k}", a, b) for k, a, b in zip(("dx", "dgamma", "dbeta"), aff, (dx, dg, db))]
        ctx.same.append(("ssv_bn_apply's mask vs the fp64 gate", ma, _pack_mask(inp["gate_aff"]).to(ctx.dev)))
        if c["acc"] == "null":
            nul = ctx.out("aff_dx", (m, ch))
            ws, _ = ctx.ws("workspace", wsb)
            L.call("ssv_bn_relu_bwd_affine", m, ch, P(dy), P(x), P(gamma), P(mean_in), P(invstd_in), P(scale), P(shift), P(nul), None, None, 0, P(ws), wsb, L.stream())
            ctx.same.append(("ssv_bn_relu_bwd_affine without dgamma / dbeta: dx", nul, aff[0]))
        out.update({"aff_dx": aff[0], "aff_dgamma": aff[1], "aff_dbeta": aff[2]})

    # ---- column sum
    def colsum(prior, acc):
        cs = ctx.out("colsum", (ch,), prior=prior)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_colsum", m, ch, P(x), P(cs), acc, P(ws), wsb, L.stream())
        return cs
    out["colsum"] = colsum(inp["cs0"], 1) if c["acc"] == "acc" else colsum(None, 0)
    ctx.same.append(("ssv_colsum, accumulate on a zero prior vs overwrite", colsum(torch.zeros(ch), 1), colsum(None, 0)))
    return out


def _part_gpu(c, inp, ctx):
    from ssv_amd import ops
    L = _lib()
    P = L.ptr
    m, ch, relu, mom = c["M"], c["C"], int(bool(c["relu"])), c["momentum"]
    x, gamma, beta, pmean, pm2 = (ctx.up(nm, inp[nm]) for nm in ("x", "gamma", "beta", "pmean", "pm2"))
    res = ctx.up("res", inp["res"]) if c["res"] else None
    rpg = ops._rows_per_group((pmean, pm2) if c["rpg"] == 64 else (pmean, pm2, c["rpg"]))
    assert rpg == c["rpg"] and pmean.shape[0] == cdiv(m, rpg)
    wsb = L.load().ssv_bn_workspace_bytes(m, ch)
    assert wsb == 4 * ws_floats(m, ch), "bn_plan as restated in this file is not the library's"

    def running(tag):
        if mom is None:
            return None, None, None
        return ctx.out("running_mean" + tag, (ch,), prior=inp["rm0"]), ctx.out("running_var" + tag, (ch,), prior=inp["rv0"]), ctx.ints("nbt" + tag, [7], torch.int64)

    def whole():
        y, mean, invstd = ctx.out("y", (m, ch)), ctx.out("mean", (ch,)), ctx.out("invstd", (ch,))
        mask = ctx.bytes("mask", m * ch // 4) if relu else None
        rm, rv, nbt = running("")
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_fwd_partials", m, ch, P(x), P(pmean), P(pm2), rpg, P(gamma), P(beta), P(res), relu, EPS, 0.0 if mom is None else mom, P(rm), P(rv), P(nbt),
               P(y), P(mask), P(mean), P(invstd), P(ws), wsb, L.stream())
        scale, shift = ws[:ch].clone(), ws[ch:2 * ch].clone()
        return {k: v for k, v in (("y", y), ("mean", mean), ("invstd", invstd), ("mask", mask), ("running_mean", rm), ("running_var", rv), ("nbt", nbt)) if v is not None}, scale, shift
    (got, scale_w, shift_w), (again, _, _) = whole(), whole()
    ctx.same += [(f"ssv_bn_train_fwd_partials, second call: {k}", got[k], again[k]) for k in got]
    # the same in two calls
    mean, invstd, scale, shift = (ctx.out(nm, (ch,)) for nm in ("mean", "invstd", "scale", "shift"))
    rm, rv, nbt = running(" (finalize)")
    ws, _ = ctx.ws("workspace", wsb)
    L.call("ssv_bn_stats_finalize", m, ch, P(pmean), P(pm2), rpg, P(gamma), P(beta), EPS, 0.0 if mom is None else mom, P(rm), P(rv), P(nbt), P(mean), P(invstd),
           P(scale), P(shift), P(ws), wsb, L.stream())
    y = ctx.out("y (ssv_bn_apply)", (m, ch))
    mask = ctx.bytes("mask (ssv_bn_apply)", m * ch // 4) if relu else None
    L.call("ssv_bn_apply", m, ch, P(x), P(scale), P(shift), P(res), None, None, relu, P(y), P(mask), L.stream())
    two = {k: v for k, v in (("y", y), ("mean", mean), ("invstd", invstd), ("mask", mask), ("running_mean", rm), ("running_var", rv), ("nbt", nbt)) if v is not None}
    ctx.same += [(f"ssv_bn_train_fwd_partials vs ssv_bn_stats_finalize + ssv_bn_apply: {k}", got[k], two[k]) for k in got]
    ctx.same += [("scale in the workspace vs ssv_bn_stats_finalize's", scale_w, scale), ("shift in the workspace vs ssv_bn_stats_finalize's", shift_w, shift)]
    if mom is not None:
        assert int(got["nbt"]) == 8 and int(nbt) == 8
    got.pop("nbt", None)
    got.update({"scale": scale, "shift": shift})
    if c["own"]:                                                        # (e): the partials of bn_stats_k's own partition - side by side with ssv_bn_train_fwd
        fy, fmean, finv = ctx.out("fwd_y", (m, ch)), ctx.out("fwd_mean", (ch,)), ctx.out("fwd_invstd", (ch,))
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_train_fwd", m, ch, P(x), P(gamma), P(beta), P(res), relu, EPS, 0.0, None, None, None, P(fy), None, P(fmean), P(finv), P(ws), wsb, L.stream())
        got.update({"fwd_y": fy, "fwd_mean": fmean, "fwd_invstd": finv})
    return got


def _apply_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    m, ch, relu = c["M"], c["C"], int(bool(c["relu"]))
    x, scale, shift = (ctx.up(nm, inp[nm]) for nm in ("x", "scale", "shift"))
    res = ctx.up("res", inp["res"]) if c["res"] else None
    rs, rh = (ctx.up("rscale", inp["rscale"]), ctx.up("rshift", inp["rshift"])) if c["res"] == 2 else (None, None)

    def run(want_mask):
        y = ctx.out("y", (m, ch))
        mask = ctx.bytes("mask", m * ch // 4) if want_mask else None
        L.call("ssv_bn_apply", m, ch, P(x), P(scale), P(shift), P(res), P(rs), P(rh), relu, P(y), P(mask), L.stream())
        return y, mask
    y, mask = run(bool(c["mask"]))
    other, _ = run(relu and not c["mask"])
    ctx.same.append(("ssv_bn_apply with and without a mask: y", other, y))
    return {"y": y, "mask": mask} if c["mask"] else {"y": y}


def _bwdp_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    m, ch = c["M"], c["C"]
    x, g, gamma, mean, invstd, psg, psgx = (ctx.up(nm, inp[nm]) for nm in ("x", "g", "gamma", "mean_in", "invstd_in", "psum_g", "psum_gx"))
    groups = psg.shape[0]
    assert groups == cdiv(m, c["rpg"])
    wsb = L.load().ssv_bn_workspace_bytes(m, ch)
    assert wsb == 4 * ws_floats(m, ch), "bn_plan as restated in this file is not the library's"

    def full(mode):
        dx = ctx.out("dx", (m, ch))
        dg, db, acc = _grads(ctx, c, inp, mode, ch)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_bwd_from_partials", m, ch, P(g), P(x), P(gamma), P(mean), P(invstd), P(psg), P(psgx), groups, P(dx), P(dg), P(db), acc, P(ws), wsb, L.stream())
        return {k: v for k, v in (("dx", dx), ("dgamma", dg), ("dbeta", db)) if v is not None}

    def coef(mode):
        co = ctx.out("coef", (4, ch))
        dg, db, acc = _grads(ctx, c, inp, mode, ch, " (coef)")
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_bwd_coef", m, ch, P(gamma), P(mean), P(invstd), P(psg), P(psgx), groups, P(co), P(dg), P(db), acc, P(ws), wsb, L.stream())
        return {k: v for k, v in (("coef", co), ("dgamma", dg), ("dbeta", db)) if v is not None}
    mode = c["acc"]
    got, again, co = full(mode), full(mode), coef(mode)
    ctx.same += [(f"ssv_bn_bwd_from_partials, second call: {k}", got[k], again[k]) for k in got]
    ctx.same += [(f"ssv_bn_bwd_coef vs ssv_bn_bwd_from_partials: {k}", co[k], got[k]) for k in ("dgamma", "dbeta") if k in got]
    zero, plain = full("zero"), full("ow")
    ctx.same += [(f"accumulate on a zero prior vs overwrite: {k}", zero[k], plain[k]) for k in zero]
    ctx.same += [("coef[1] is the saved mean", co["coef"][1], mean), ("dx with and without dgamma / dbeta", plain["dx"], got["dx"])]
    if mode == "null":
        got.update({"dgamma": plain["dgamma"], "dbeta": plain["dbeta"]})
    k = co["coef"].double().cpu()
    got.update({"coef": co["coef"], "dx_coef": k[0] * inp["g"].double() + k[2] * (inp["x"].double() - k[1]) + k[3]})
    return got


def _stem_gpu(c, inp, ctx):
    from ssv_amd import nn as hnn
    L = _lib()
    P = L.ptr
    n, h, w, ch = c["shape"]
    ho, wo, m = (h - 1) // 2 + 1, (w - 1) // 2 + 1, n * h * w
    y, gamma, scale, shift, mean, invstd = (ctx.up(nm, inp[nm]) for nm in ("y", "gamma", "scale_in", "shift_in", "mean_in", "invstd_in"))

    def fwd(keep):
        out, am = ctx.out("stem_out", (n, ho, wo, ch)), ctx.bytes("argmax", n * ho * wo * ch).view(n, ho, wo, ch)
        xmax = ctx.out("xmax", (n, ho, wo, ch)) if keep else None
        L.call("ssv_bn_relu_maxpool_fwd", n, h, w, ch, P(y), P(scale), P(shift), P(out), P(am), P(xmax), L.stream())
        return out, am, xmax
    out, am, xmax = fwd(True)
    if not c["fwd_only"]:
        out2, am2, _ = fwd(False)
        ctx.same += [("ssv_bn_relu_maxpool_fwd with and without xmax: out", out2, out), ("... arg-max", am2, am)]
    ya = ctx.out("y (ssv_bn_apply)", (m, ch))
    L.call("ssv_bn_apply", m, ch, P(y), P(scale), P(shift), None, None, None, 1, P(ya), None, L.stream())
    py, pam = ctx.out("pooled", (n, ho, wo, ch)), ctx.bytes("argmax (ssv_maxpool3x3s2_fwd)", n * ho * wo * ch).view(n, ho, wo, ch)
    L.call("ssv_maxpool3x3s2_fwd", n, h, w, ch, P(ya), P(py), P(pam), L.stream())
    ctx.same += [("ssv_bn_relu_maxpool_fwd vs ssv_bn_apply + ssv_maxpool3x3s2_fwd: out", out, py), ("... arg-max", am, pam)]
    idx = _slots_to_idx(am.cpu(), h, w)
    picked = inp["y"].permute(0, 3, 1, 2).reshape(n, ch, -1).gather(2, idx.view(n, ch, -1)).view(n, ch, ho, wo).permute(0, 2, 3, 1).contiguous()
    ctx.same.append(("xmax vs y at the kernel's own arg-max", xmax.cpu(), picked))
    del idx, picked
    if c["fwd_only"]:
        return {"stem_out": out}
    dpool, am_in, xmax_in = ctx.up("dpool", inp["dpool"]), ctx.up("am_in", inp["am_in"]), ctx.up("xmax_in", inp["xmax_in"])
    wsb = L.load().ssv_bn_workspace_bytes(m, ch)
    assert wsb == 4 * ws_floats(m, ch), "bn_plan as restated in this file is not the library's"

    def bwd(xm, mode, tag=""):
        dy = ctx.out("stem_dy" + tag, (n, h, w, ch))
        dg, db, acc = _grads(ctx, c, inp, mode, ch, tag)
        ws, _ = ctx.ws("workspace", wsb)
        L.call("ssv_bn_relu_maxpool_bwd", n, h, w, ch, P(dpool), P(am_in), P(y), P(xm), P(gamma), P(mean), P(invstd), P(scale), P(shift), P(dy), P(dg), P(db), acc,
               P(ws), wsb, L.stream())
        return {k: v for k, v in (("stem_dy", dy), ("stem_dgamma", dg), ("stem_dbeta", db)) if v is not None}
    if c["refused"]:
        dy, ws = ctx.out("stem_dy", (n, h, w, ch), nan_ok=True), ctx.ws("workspace", wsb)[0]
        _refused("ssv_bn_relu_maxpool_bwd", n, h, w, ch, P(dpool), P(am_in), P(y), None, P(gamma), P(mean), P(invstd), P(scale), P(shift), P(dy), None, None, 0,
                 P(ws), wsb, L.stream())
        assert bool(torch.isnan(dy).all()), "a refused call wrote its output"
        bn = hnn.HipBatchNorm(ch, eps=EPS, momentum=MOMENTUM).to(ctx.dev)
        with torch.no_grad():
            bn.weight.copy_(inp["gamma"])
            bn.bias.copy_(inp["beta"])
        xin = y.clone()
        xin._bn_partials = (ctx.up("pmean", inp["pmean"]), ctx.up("pm2", inp["pm2"]))
        tape = hnn.Tape(xin, True)                                      # with a tape: the fused route would record ONE op whose backward the library refuses
        routed = hnn.bn_relu_maxpool(tape, xin, bn)
        assert "_bn_partials" not in xin.__dict__ and int(bn.num_batches_tracked) == 1
        assert len(tape.ops) == 2, f"nn.bn_relu_maxpool recorded {len(tape.ops)} op(s): not the BatchNorm + max-pool route"
        dx = tape.backward(routed, dpool.clone())
        return {"nn_out": routed, "nn_dy": dx, "nn_dgamma": bn.weight.grad, "nn_dbeta": bn.bias.grad}
    mode = c["acc"]
    got, again = bwd(None, mode), bwd(None, mode)
    ctx.same += [(f"ssv_bn_relu_maxpool_bwd, second call: {k}", got[k], again[k]) for k in got]
    zero, plain = bwd(None, "zero"), bwd(None, "ow")
    ctx.same += [(f"ssv_bn_relu_maxpool_bwd, accumulate on a zero prior vs overwrite: {k}", zero[k], plain[k]) for k in zero]
    # the unfused route on the same arg-max: bit-identical
    dfull = ctx.out("dy (ssv_maxpool3x3s2_bwd)", (n, h, w, ch))
    L.call("ssv_maxpool3x3s2_bwd", n, h, w, ch, P(dpool), P(am_in), P(dfull), L.stream())
    dx = ctx.out("dx (ssv_bn_train_bwd)", (m, ch))
    dg, db, acc = _grads(ctx, c, inp, "ow", ch, " (ssv_bn_train_bwd)")
    ws, _ = ctx.ws("workspace", wsb)
    L.call("ssv_bn_train_bwd", m, ch, P(dfull), P(ya), None, P(y), P(gamma), P(mean), P(invstd), 1, P(dx), None, P(dg), P(db), acc, P(ws), wsb, L.stream())
    ctx.same += [("ssv_bn_relu_maxpool_bwd vs ssv_maxpool3x3s2_bwd + ssv_bn_train_bwd: dy", plain["stem_dy"].view(m, ch), dx),
                 ("... dgamma", plain["stem_dgamma"], dg), ("... dbeta", plain["stem_dbeta"], db)]
    pooled = bwd(xmax_in, mode, "_x")
    if "stem.fallback" in c.labels:
        ctx.same += [(f"xmax given but dropped vs xmax NULL: {k}", pooled[k], got[k]) for k in got]
    got.update({k + "_x": v for k, v in pooled.items()})
    if mode == "null":
        px = bwd(xmax_in, "ow", "_x")
        got.update({"stem_dgamma": plain["stem_dgamma"], "stem_dbeta": plain["stem_dbeta"], "stem_dgamma_x": px["stem_dgamma"], "stem_dbeta_x": px["stem_dbeta"]})
        ctx.same.append(("xmax path, dy with and without dgamma / dbeta", px["stem_dy"], pooled["stem_dy"]))
    got["stem_out"] = out
    return got


def _pool_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, h, w, ch = c["shape"]
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x, dy = ctx.up("x", inp["x"]), ctx.up("dy", inp["dy"])
    y, am = ctx.out("pool_y", (n, ho, wo, ch), nan_ok=c["mode"] == "nonfinite"), ctx.bytes("pool_am", n * ho * wo * ch).view(n, ho, wo, ch)
    L.call("ssv_maxpool3x3s2_fwd", n, h, w, ch, P(x), P(y), P(am), L.stream())
    if c["mode"] == "nonfinite":
        return {"pool_y": y, "pool_am": am}
    dx = ctx.out("pool_dx", (n, h, w, ch))
    L.call("ssv_maxpool3x3s2_bwd", n, h, w, ch, P(dy), P(am), P(dx), L.stream())
    single = _pool_terms(c, inp) <= 1                                   # (c): at most one term - no sum, no order
    exact = _scatter(inp["dy"], _pool_nhwc(inp["x"])[2], h, w)
    assert _same(dx.cpu()[single], exact[single]), "a pixel that receives at most one term is not exact"
    return {"pool_y": y, "pool_am": am, "pool_dx": dx}


def _gap_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, hw, ch = c["shape"]
    x, dy = ctx.up("x", inp["x"]), ctx.up("dy", inp["dy"])
    y, dx = ctx.out("gap_y", (n, ch)), ctx.out("gap_dx", (n, hw, ch))
    L.call("ssv_gap_fwd", n, hw, ch, P(x), P(y), L.stream())
    L.call("ssv_gap_bwd", n, hw, ch, P(dy), P(dx), L.stream())
    if hw <= 64:                                                        # gap_fwd_k: up to 64 terms the sum is the plain serial one, bit for bit
        serial = torch.zeros(n, ch)
        for j in range(hw):
            serial += inp["x"][:, j]
        ctx.same.append(("HW <= 64: the serial fp32 sum / HW", y.cpu(), serial / hw))
    if hw == 1:
        ctx.same += [("HW = 1: the mean is the element", y, x.view(n, ch)), ("HW = 1: dx is dy", dx.view(n, ch), dy)]
    return {"gap_y": y, "gap_dx": dx}


def _layout_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, ch, h, w = c["shape"]
    a, b = ctx.up("nchw_in", inp["nchw_in"]), ctx.up("nhwc_in", inp["nhwc_in"])
    nhwc, nchw, back = ctx.out("nhwc", (n, h, w, ch)), ctx.out("nchw", (n, ch, h, w)), ctx.out("round trip", (n, ch, h, w))
    L.call("ssv_nchw_to_nhwc", n, ch, h, w, P(a), P(nhwc), L.stream())
    L.call("ssv_nhwc_to_nchw", n, ch, h, w, P(b), P(nchw), L.stream())
    L.call("ssv_nhwc_to_nchw", n, ch, h, w, P(nhwc), P(back), L.stream())
    ctx.same.append(("ssv_nhwc_to_nchw(ssv_nchw_to_nhwc(x)) is x", back, a))
    return {"nhwc": nhwc, "nchw": nchw}


def _pad_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    npix, cin, cout = c["npix"], c["cin"], c["cout"]
    t = ctx.up("t", inp["t"])
    if cin == cout:
        out = ctx.out("pad", (npix, cout), nan_ok=True)
        _refused("ssv_pad_channels", npix, cin, cout, P(t), P(out), 0, L.stream())
        assert bool(torch.isnan(out).all()), "a refused call wrote its output"
        return {"pad": t}
    out = ctx.out("pad", (npix, cout), prior=inp["prior"] if c["acc"] else None)
    L.call("ssv_pad_channels", npix, cin, cout, P(t), P(out), int(bool(c["acc"])), L.stream())
    return {"pad": out}


def _group_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    k, r, s, cg, groups = c["K"], c["R"], c["S"], c["Cg"], c["groups"]
    w, dwd = ctx.up("w", inp["w"]), ctx.up("dwd", inp["dwd"])
    wd, back = ctx.out("wd", (k, r, s, cg * groups)), ctx.out("round trip", (k, r, s, cg))
    wg = ctx.out("wg", (k, r, s, cg), prior=inp["prior"] if c["acc"] else None)
    L.call("ssv_group_expand", k, r, s, cg, groups, P(w), P(wd), L.stream())
    L.call("ssv_group_extract", k, r, s, cg, groups, P(dwd), P(wg), int(bool(c["acc"])), L.stream())
    L.call("ssv_group_extract", k, r, s, cg, groups, P(wd), P(back), 0, L.stream())
    ctx.same.append(("ssv_group_extract(ssv_group_expand(w)) is w", back, w))
    return {"wd": wd, "wg": wg}


def _ftrans_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    k, r, s, ch = c["K"], c["R"], c["S"], c["C"]
    w = ctx.up("w", inp["w"])
    wt, back = ctx.out("wt", (ch, r, s, k)), ctx.out("round trip", (k, r, s, ch))
    L.call("ssv_filter_transpose", k, r, s, ch, P(w), P(wt), L.stream())
    L.call("ssv_filter_transpose", ch, r, s, k, P(wt), P(back), L.stream())
    ctx.same.append(("ssv_filter_transpose twice is the identity", back, w))
    return {"wt": wt}


GPU = {"bn": _bn_gpu, "part": _part_gpu, "apply": _apply_gpu, "bwdp": _bwdp_gpu, "stem": _stem_gpu, "pool": _pool_gpu, "gap": _gap_gpu, "layout": _layout_gpu,
       "pad": _pad_gpu, "group": _group_gpu, "ftrans": _ftrans_gpu}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_kernel_against_fp64(dev, case):
    _, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    ctx = Ctx(dev)
    got = GPU[case.kind](case, inp, ctx)
    torch.cuda.synchronize()
    assert set(got) == set(r64), f"{case.id}: {sorted(set(got) ^ set(r64))}"
    nonfinite = "pool.nonfinite" in case.labels
    fails, rec = [], REPORT.setdefault(case.id, {})
    for name, ref64 in r64.items():
        g = got[name].detach().reshape(ref64.shape).cpu()
        fam = FAMILY[name]
        if fam == "exact":
            if not _same(g, r32[name]):
                fails.append(f"{case.id} {name}: not bit-identical to the reference ({int((g != r32[name]).sum())} of {g.numel()} elements differ)")
            continue
        assert nonfinite or torch.isfinite(g).all(), f"{case.id} {name}: non-finite values"
        (eg, mg), (er, mr) = _err(g, ref64), _err(r32[name], ref64)
        rec[name] = {"e_got": eg, "e_ref32": er, "m_got": mg, "m_ref32": mr}
        print(f"{case.id} {name}: e {eg:.3e} (ref32 {er:.3e}) m {mg:.3e} (ref32 {mr:.3e})")
        if not (eg <= FACTOR[fam] * er + FLOOR[fam] and mg <= FACTOR[fam] * mr + FLOOR[fam]):
            fails.append(f"{case.id} {name}: e {eg:.3e} vs ref32 {er:.3e}, m {mg:.3e} vs ref32 {mr:.3e} (FACTOR {FACTOR[fam]:g}, FLOOR {FLOOR[fam]:.2e})")
        if name in PAIRS:                                                # (e): "rounding-level" - within the bar of the other path as well
            other = got[PAIRS[name]].detach().reshape(ref64.shape).cpu().double()
            eb = float((g.double() - other).norm() / ref64.norm().clamp_min(1e-300))
            print(f"{case.id} {name} vs {PAIRS[name]}: {eb:.3e}")
            if not eb <= FACTOR[fam] * er + FLOOR[fam]:
                fails.append(f"{case.id} {name}: {eb:.3e} from {PAIRS[name]}, ref32 {er:.3e}")
    ctx.verify(case.id)
    assert not fails, "\n".join(fails)
