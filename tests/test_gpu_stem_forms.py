"""Every launch form of the 3-channel image stem (csrc/conv_mfma.hip: stem_fwd_rows_k, the row-taps forward conv_fwd_k<256, 64, 4, 1, 24, ..., 2>,
stem_wgrad_rows_k, the row-taps weight gradient conv_wgrad_k<64, 192, 2, 2, 32, true, 3>) and of the image padded to 4 channels (the C == 4 selections of
launch_fwd) against an fp64 evaluation, at plans with several iterations / rows per workgroup - the plans the training step runs.

Each case of CASES names its family, the branch labels it targets and a geometry (N, H, W, K, R = S, stride, pad).  The inputs are drawn on the CPU from a
generator seeded by the case id (images 0.5 + N(0, 1): not constant, every border pixel matters; weights N(0, 1) (27 R S)^-1/2).  TAU, U and GUARD are
tests/test_gpu_conv_forms.py's (imported; 16 per family from the fp32-accumulation argument stated there).  Every case is held to:

  (a) element-wise: |got - ref64| <= TAU * 2^-24 * A + floor; ref64 is F.conv2d (or its weight gradient) in float64 on the CPU from the same fp32 inputs, A the
      same operation on the absolute values of the operands.  y, dwrows (all K R 24 entries) and the C == 4 outputs;
  (b) the stem has no bf16-piece form: every case runs under ops.arithmetic("f32") and ops.arithmetic("bf16x3"), the two results are bit-identical and
      ssv_conv_arithmetic(desc, 0 / 2) answers SSV_ARITH_F32_MFMA for C == 3 (the C == 4 weight gradient HAS a one-accumulator form: there the bf16x3
      relative l2 error against fp64 stays <= 1.05 x the fp32-MFMA one + 1e-9, test_gpu_conv_forms' bar);
  (d) statistics partials, EVERY group: the group size is ssv_stem_conv_fwd_stats_rows_per_group(desc), the count ceil(M / size); each group's mean against
      the fp64 mean of the rows the kernel itself wrote (y.double()), each M2 against their fp64 centred sum of squares.  The 64-row groups of the row-taps
      kernel (and of the C == 4 statistics epilogue) follow _stats_partials' error model of test_gpu_conv_forms.py (that kernel sums around the group's
      first row).  The rows-in-LDS kernel is two-pass per wave plus an equal-count merge: its M2 is bounded by TAU["partials"] * 2^-24 * sum over the group
      of (|y| + |mean|)^2, which bounds every intermediate, its mean by TAU["partials"] * 2^-24 * mean |y| (rule (a) on a mean).  Then ops.bn_stats_finalize
      on the partials against the fp64 mean and inverse standard deviation of the whole map under the bn-forward rule of test_gpu_bn_pool_kernels.py
      (e(got) <= FACTOR * e(ref32) + FLOOR, and the same for the max-norm figure m; ref32 = the same lines in float32 on the CPU);
  (e) guards: y, pmean, pm2, dwrows and the workspace of exactly ssv_stem_conv_wgrad_workspace_bytes(desc) bytes live in NaN-prefilled buffers with GUARD
      floats of NaN behind them - nothing of an output stays NaN, the guards stay NaN, the padding columns e >= 3 S of dwrows are exact zeros (the workspace is sized for
      the larger of the two kernels' plans, so the launched one may leave a part of it unwritten: only its guard is checked).  x and dy are
      16-byte aligned views into buffers with GUARD floats of NaN IN FRONT and BEHIND, and bit-identical after the call: the rows-in-LDS kernels read the
      image with plain global float4 loads, the row-taps kernels move the windows of the first and last pixels of the batch inside the tensor
      (straddle_off / straddle_fix) - nothing outside [x, x + N H W 3) may reach a result (it would arrive as a NaN);
  (f) bitwise identities: a second identical call gives the first call's bits (forward, partials, weight gradient - its reduce is fixed-order); y with
      statistics == y without; y[n] of a batch == y of a launch on image n alone for n = 0, the middle and the last image, on both forward kernels (the
      per-pixel MFMA order depends on the map, not the batch: on the multi-iteration cases this alone pins the prefetch / store-over loop; on the
      rows-in-LDS kernel the image's partials are compared too); ops.stem_conv_fwd / ops.stem_conv_wgrad == the direct C-ABI calls.

Branches (label, the function that selects it, what the case reaches) - test_case_table_covers_every_documented_branch keeps CASES honest, and
test_case_shapes_have_the_plan_their_label_claims holds every case to the plan facts stated here, from a restatement of the four selection functions whose
constants are read from the text of conv_mfma.hip (a retune fails the table instead of silently moving a case to another branch):

  sfwd.rows_w7             conv_mfma.hip:stem_fwd_rows_rpi   (1, 4, 224, 64, 7, 2, 3): rpi 2, 224 px, 7 waves, 1 iteration, 9 staged rows
  sfwd.rows_w6             conv_mfma.hip:stem_fwd_rows_rpi   (2, 8, 192, 64, 7, 2, 3): rpi 2, 192 px, the seventh wave idle (the merge divides by 6)
  sfwd.rows_rpi3           conv_mfma.hip:stem_fwd_rows_rpi   (3, 6, 64, 64, 3, 1, 1): rpi 3, stride 1, 5 staged rows of 9
  sfwd.rows_rpi4_s2        conv_mfma.hip:stem_fwd_rows_rpi   (2, 8, 96, 64, 3, 2, 1): rpi 4, stride 2, R 3, 9 staged rows
  sfwd.rows_r5             conv_mfma.hip:stem_fwd_rows_rpi   (2, 4, 112, 64, 5, 1, 2): R 5, 8 steps per filter row, the odd 3 S padded with a zero weight
  sfwd.rows_multi          conv_mfma.hip:ssv_stem_conv_fwd   (257, 8, 224, 64, 7, 2, 3): 514 iterations, 2 per workgroup, 257 workgroups; Ho / rpi = 2, so every iteration touches the top or bottom padding rows of an image
  sfwd.rows_multi_ragged   conv_mfma.hip:ssv_stem_conv_fwd   (513, 6, 32, 64, 3, 1, 1): rpi 6, 6 waves, 513 iterations, 2 per workgroup, the last workgroup 1
  sfwd.taps                conv_mfma.hip:ssv_stem_conv_fwd   (5, 33, 31, 64, 7, 2, 3), (2, 9, 11, 68, 3, 1, 1): row-taps, M % 256 != 0, odd sizes; K 68: the second column tile ragged
  sfwd.taps_k3tiles        conv_mfma.hip:ssv_stem_conv_fwd   (2, 13, 7, 132, 7, 2, 3): three column tiles
  sfwd.taps_s8             conv_mfma.hip:ssv_stem_conv_fwd   (3, 16, 12, 64, 8, 2, 3): S = 8, all 24 floats of a filter row real
  sfwd.taps_wide           conv_mfma.hip:stem_fwd_rows_rpi   refused: (1, 8, 228, 64, 7, 2, 3) Wo 114, no rpi with rpi Wo % 32 == 0; (2, 8, 448, 64, 7, 2, 3) padl + 3 W > SF_ROWF
  sfwd.taps_straddle       conv_mfma.hip:straddle_off        every sfwd.taps* case: pad > 0, the first window starts before x and the last ends past it; the first and last output pixel are compared
  swg.rows_one             conv_mfma.hip:stem_rows_ok        (7, 20, 20, 64, 7, 2, 3), (2, 4, 112, 64, 5, 1, 2), (3, 6, 64, 64, 3, 1, 1): 1 row per workgroup; NCOL 168 / 120 / 72 (the col >= NCOL skip, the zero LDS row)
  swg.rows_multi           conv_mfma.hip:stem_rows_plan      (257, 8, 224, 64, 7, 2, 3), (193, 8, 8, 64, 7, 2, 3): 2 rows per workgroup, even; Wo 112 (the maximum) and Wo 4
  swg.rows_multi_ragged    conv_mfma.hip:stem_rows_plan      (513, 6, 32, 64, 3, 1, 1): G 3078, 5 rows per workgroup, 616 workgroups, the last one 3 rows
  swg.taps                 conv_mfma.hip:plan_stem_wgrad     (2, 8, 10, 64, 7, 2, 3): Wo odd refuses the rows kernel; 1 tile, 1 chunk, M % 32 != 0
  swg.taps_nsplit          conv_mfma.hip:plan_stem_wgrad     (5, 33, 31, 64, 7, 2, 3), (1, 8, 228, 64, 7, 2, 3): 6 and 2 chunks, the last one short
  swg.taps_tiles           conv_mfma.hip:plan_stem_wgrad     (2, 13, 7, 132, 7, 2, 3), (2, 9, 11, 68, 3, 1, 1): 3 and 2 column tiles (ragged)
  c4.fwd_narrow            conv_mfma.hip:launch_fwd          C 4, (2, 13, 7, 64, 7, 2, 3): tap-vector gather, 256 x 64 tile; 49 taps = 7 k-tiles with a 1-tap tail
  c4.fwd_wide              conv_mfma.hip:launch_fwd          C 4, (2, 9, 11, 132, 3, 1, 1): 128 x 128 tile; 9 taps = 2 k-tiles
  c4.fwd_stats             conv_mfma.hip:launch_fwd          the same two through ssv_conv2d_fwd_stats: partials under (d), ssv_conv2d_fwd_stats_groups groups
  c4.wgrad                 conv_mfma.hip:wgrad_impl          C 4, (3, 20, 20, 64, 7, 2, 3) through ssv_conv2d_wgrad: the padded input channel's column is exactly zero
  stem.refused             conv_mfma.hip:ssv_stem_conv_wgrad K = 66; S = 9; a workspace one byte short; pmean without pm2: an error status and a message from ssv_last_error, outputs untouched (still NaN)
  stem.host                nn.py:stem_conv                   (4, 16, 16, 64, 7, 2, 3) with a tape, nn._ROW_STEM True and False, bn_stats on, a non-zero prior in the weight's gradient: y, _bn_partials and prior + dW under (a) and (d); and (3, 16, 12, 64, 8, 2, 3), whose 8-tap rows fill their 24 floats (ops.stem_weight_rows / the backward must not ask ssv_pad_channels for 24 -> 24, which it refuses)

Selections this file does not reach (UNREACHED; the table test lists them instead of omitting them): the N H W 12 >= 2^31 byte clauses of stem_fwd_rows_rpi
and stem_rows_ok need an image batch of 2 GiB, far beyond a test's size.

Measured on an MI355X: profiles/stem_forms_report.json (written by this file under SSV_STEM_REPORT=<path>) and DESIGN.md section 2.
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

from test_gpu_bn_pool_kernels import FACTOR, FLOOR
from test_gpu_conv_forms import GUARD, TAU, U, defines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-supervised-vision_amd", "csrc")
WORST = {}                                                                # family -> worst |err| / bound seen (SSV_STEM_REPORT)
UNREACHED = {"sfwd.bytes_2gib": "stem_fwd_rows_rpi: N H W 12 >= 2^31 refuses the rows-in-LDS forward",
             "swg.bytes_2gib": "stem_rows_ok: N H W 12 >= 2^31 refuses the rows-in-LDS weight gradient"}


class Case:
    def __init__(self, kind, labels, geom, c=3, **opt):
        self.kind, self.labels, self.geom, self.c, self.opt = kind, tuple(labels.split()), geom, c, opt
        n, h, w, k, r, s, pad = geom
        self.id = f"{kind}-N{n}H{h}W{w}C{c}K{k}R{r}s{s}p{pad}" + "".join(f"-{a}{b}" for a, b in sorted(opt.items()))
        self.ho, self.wo = (h + 2 * pad - r) // s + 1, (w + 2 * pad - r) // s + 1
        self.m = n * self.ho * self.wo


# geom = (N, H, W, K, R (= S), stride, pad)
CASES = [
    Case("stem", "sfwd.rows_w7", (1, 4, 224, 64, 7, 2, 3)),
    Case("stem", "sfwd.rows_w6", (2, 8, 192, 64, 7, 2, 3)),
    Case("stem", "sfwd.rows_rpi3 swg.rows_one", (3, 6, 64, 64, 3, 1, 1)),
    Case("stem", "sfwd.rows_rpi4_s2", (2, 8, 96, 64, 3, 2, 1)),
    Case("stem", "sfwd.rows_r5 swg.rows_one", (2, 4, 112, 64, 5, 1, 2)),
    Case("stem", "sfwd.rows_multi swg.rows_multi", (257, 8, 224, 64, 7, 2, 3)),
    Case("stem", "sfwd.rows_multi_ragged swg.rows_multi_ragged", (513, 6, 32, 64, 3, 1, 1)),
    Case("stem", "sfwd.taps sfwd.taps_straddle swg.taps_nsplit", (5, 33, 31, 64, 7, 2, 3)),
    Case("stem", "sfwd.taps sfwd.taps_straddle swg.taps_tiles", (2, 9, 11, 68, 3, 1, 1)),
    Case("stem", "sfwd.taps_k3tiles sfwd.taps_straddle swg.taps_tiles", (2, 13, 7, 132, 7, 2, 3)),
    Case("stem", "sfwd.taps_s8 sfwd.taps_straddle", (3, 16, 12, 64, 8, 2, 3)),
    Case("stem", "sfwd.taps_wide sfwd.taps_straddle swg.taps_nsplit", (1, 8, 228, 64, 7, 2, 3)),
    Case("stem", "sfwd.taps_wide sfwd.taps_straddle", (2, 8, 448, 64, 7, 2, 3)),
    Case("stem", "swg.rows_one", (7, 20, 20, 64, 7, 2, 3)),
    Case("stem", "swg.rows_multi", (193, 8, 8, 64, 7, 2, 3)),
    Case("stem", "swg.taps", (2, 8, 10, 64, 7, 2, 3)),
    Case("c4", "c4.fwd_narrow c4.fwd_stats", (2, 13, 7, 64, 7, 2, 3), c=4),
    Case("c4", "c4.fwd_wide c4.fwd_stats", (2, 9, 11, 132, 3, 1, 1), c=4),
    Case("c4wgrad", "c4.wgrad", (3, 20, 20, 64, 7, 2, 3), c=4),
    Case("refused", "stem.refused", (2, 12, 12, 66, 7, 2, 3), what="k66"),
    Case("refused", "stem.refused", (2, 12, 12, 64, 9, 2, 4), what="s9"),
    Case("refused", "stem.refused", (2, 12, 12, 64, 7, 2, 3), what="ws_short"),
    Case("refused", "stem.refused", (2, 12, 12, 64, 7, 2, 3), what="pmean_only"),
    Case("host", "stem.host", (4, 16, 16, 64, 7, 2, 3), row_stem=1),
    Case("host", "stem.host", (4, 16, 16, 64, 7, 2, 3), row_stem=0),
    Case("host", "stem.host", (3, 16, 12, 64, 8, 2, 3), row_stem=1),                           # 3 S == 24: the filter rows need no padding, dW no unpadding
]
FWD_CASES = [c for c in CASES if c.kind == "stem" and any(b.startswith("sfwd.") for b in c.labels)]
WG_CASES = [c for c in CASES if c.kind == "stem" and any(b.startswith("swg.") for b in c.labels)]


# ============================================================================================================= the selection functions, restated
def _src():
    with open(os.path.join(CSRC, "conv_mfma.hip")) as f:
        return f.read()


def _const(src, pattern):
    m = re.findall(pattern, src)
    assert len(m) == 1, f"conv_mfma.hip: {pattern!r} matches {len(m)} times - the selection code changed, restate it here"
    return int(m[0])


_K = {}


def consts():
    """The constants of the four selection functions, read from the text of conv_mfma.hip."""
    if not _K:
        s = _src()
        for name in ("SF_ROWS", "SF_ROWF", "SF_K", "SF_MAXSTEPS", "SR_R", "SR_ROWF", "SR_WO", "SR_K"):
            _K[name] = _const(s, r"\b%s = (\d+)" % name)
        _K["SF_PIX_MAX"] = _const(s, r"for \(int r = 1; r \* d->Wo <= (\d+); \+\+r\)")
        _K["SF_PIX_MIN"] = _const(s, r"return best \* d->Wo >= (\d+) \? best : 0;")
        _K["SF_ROUND"] = _const(s, r"const int ipw = \(int\)cdiv64\(iters, (\d+)\);")
        _K["SR_ROUND"] = _const(s, r"r\.rows_per_wg = \(int\)cdiv64\(G, (\d+)\);")
        _K["WG_ROUND"] = _const(s, r"int64_t ns = (\d+) / w\.tiles;")
    return _K


def _cdiv(a, b):
    return -(-a // b)


def _fits(c, rowf):
    n, h, w, k, r, s, pad = c.geom
    padl = (pad * 3 + 3) // 4 * 4
    off = padl - pad * 3
    return padl + w * 3 <= rowf and off + (c.wo - 1) * s * 3 + 24 <= rowf and n * h * w * 12 < (1 << 31)


def stem_fwd_rows_rpi(c):
    """conv_mfma.hip:stem_fwd_rows_rpi - output rows per iteration of the rows-in-LDS forward, 0 = row-taps."""
    q = consts()
    n, h, w, k, r, s, pad = c.geom
    if not (c.c == 3 and k == q["SF_K"] and r <= 7 and r * 3 <= 24 and r * ((r * 3 + 1) // 2) <= q["SF_MAXSTEPS"] and w % 4 == 0 and _fits(c, q["SF_ROWF"])):
        return 0
    best, rr = 0, 1
    while rr * c.wo <= q["SF_PIX_MAX"]:
        if (rr * c.wo) % 32 == 0 and c.ho % rr == 0 and (rr - 1) * s + r <= q["SF_ROWS"]:
            best = rr
        rr += 1
    return best if best * c.wo >= q["SF_PIX_MIN"] else 0


def fwd_plan(c):
    """What ssv_stem_conv_fwd launches: the rows-in-LDS facts, or kernel "taps"."""
    n, h, w, k, r, s, pad = c.geom
    rpi = stem_fwd_rows_rpi(c)
    if not rpi:
        return dict(kernel="taps", rpi=0, group=64, row_tiles=_cdiv(c.m, 256), col_tiles=_cdiv(k, 64))
    iters = n * c.ho // rpi
    ipw = _cdiv(iters, consts()["SF_ROUND"])
    wgs = _cdiv(iters, ipw)
    return dict(kernel="rows", rpi=rpi, group=rpi * c.wo, pixels=rpi * c.wo, waves=rpi * c.wo // 32, iters=iters, ipw=ipw, wgs=wgs, last=iters - (wgs - 1) * ipw,
                staged=(rpi - 1) * s + r, spr=(3 * r + 1) // 2)


def stem_rows_ok(c):
    q = consts()
    n, h, w, k, r, s, pad = c.geom
    return c.c == 3 and k == q["SR_K"] and r <= q["SR_R"] and r * 3 <= 24 and w % 4 == 0 and c.wo % 2 == 0 and c.wo <= q["SR_WO"] and _fits(c, q["SR_ROWF"])


def stem_rows_plan(c):
    g = c.geom[0] * c.ho
    rpw = _cdiv(g, consts()["SR_ROUND"])
    nsplit = _cdiv(g, rpw)
    return dict(G=g, rows_per_wg=rpw, nsplit=nsplit, last=g - (nsplit - 1) * rpw, ncol=c.geom[4] * 24)


def plan_stem_wgrad(c):
    n, h, w, k, r, s, pad = c.geom
    tiles = _cdiv(k, 64) * _cdiv(r * 24, 192)
    ns = max(1, min(consts()["WG_ROUND"] // tiles, _cdiv(c.m, 256)))
    chunk = _cdiv(_cdiv(c.m, ns), 32) * 32
    nsplit = _cdiv(c.m, chunk)
    return dict(tiles=tiles, col_tiles=_cdiv(k, 64), nsplit=nsplit, chunk=chunk, last=c.m - (nsplit - 1) * chunk)


def wgrad_workspace_bytes(c):
    slab = c.geom[3] * c.geom[4] * 24 * 4
    return max(plan_stem_wgrad(c)["nsplit"] * slab, stem_rows_plan(c)["nsplit"] * slab if stem_rows_ok(c) else 0)


def _eligible_but_for_width(c):
    """the geometry passes every clause of stem_fwd_rows_rpi that does not look at the row width"""
    n, h, w, k, r, s, pad = c.geom
    return c.c == 3 and k == 64 and r <= 7 and w % 4 == 0


def _no_rpi(c):
    return not any((rr * c.wo) % 32 == 0 and c.ho % rr == 0 for rr in range(1, 224 // c.wo + 1))


# label -> the plan facts it claims (test_case_shapes_have_the_plan_their_label_claims)
PROPERTY = {
    "sfwd.rows_w7": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", rpi=2, pixels=224, waves=7, iters=1, ipw=1, staged=9),
    "sfwd.rows_w6": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", rpi=2, pixels=192, waves=6),
    "sfwd.rows_rpi3": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", rpi=3, staged=5) and c.geom[5] == 1 and consts()["SF_ROWS"] == 9,
    "sfwd.rows_rpi4_s2": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", rpi=4, staged=9) and c.geom[4:6] == (3, 2),
    "sfwd.rows_r5": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", spr=8) and c.geom[4] == 5 and (3 * c.geom[4]) % 2 == 1,
    "sfwd.rows_multi": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", iters=514, ipw=2, wgs=257, last=2) and c.ho // fwd_plan(c)["rpi"] == 2 and c.geom[6] > 0,
    "sfwd.rows_multi_ragged": lambda c: fwd_plan(c) == dict(fwd_plan(c), kernel="rows", rpi=6, waves=6, iters=513, ipw=2, last=1),
    "sfwd.taps": lambda c: fwd_plan(c)["kernel"] == "taps" and c.m % 256 != 0 and (c.geom[1] % 2 == 1 and c.geom[2] % 2 == 1) and c.geom[3] in (64, 68),
    "sfwd.taps_k3tiles": lambda c: fwd_plan(c)["kernel"] == "taps" and fwd_plan(c)["col_tiles"] == 3,
    "sfwd.taps_s8": lambda c: fwd_plan(c)["kernel"] == "taps" and c.geom[4] == 8,
    "sfwd.taps_wide": lambda c: fwd_plan(c)["kernel"] == "taps" and _eligible_but_for_width(c) and ((c.wo == 114 and _no_rpi(c) and _fits(c, consts()["SF_ROWF"]))
                                                                                                  or (c.geom[6] * 3 + 3) // 4 * 4 + 3 * c.geom[2] > consts()["SF_ROWF"]),
    "sfwd.taps_straddle": lambda c: fwd_plan(c)["kernel"] == "taps" and c.geom[6] > 0,
    "swg.rows_one": lambda c: stem_rows_ok(c) and stem_rows_plan(c)["rows_per_wg"] == 1 and stem_rows_plan(c)["ncol"] in (168, 120, 72),
    "swg.rows_multi": lambda c: stem_rows_ok(c) and stem_rows_plan(c)["rows_per_wg"] == 2 and stem_rows_plan(c)["last"] == 2 and c.wo in (consts()["SR_WO"], 4),
    "swg.rows_multi_ragged": lambda c: stem_rows_ok(c) and stem_rows_plan(c) == dict(stem_rows_plan(c), G=3078, rows_per_wg=5, nsplit=616, last=3),
    "swg.taps": lambda c: not stem_rows_ok(c) and c.wo % 2 == 1 and plan_stem_wgrad(c) == dict(plan_stem_wgrad(c), tiles=1, nsplit=1) and c.m % 32 != 0,
    "swg.taps_nsplit": lambda c: not stem_rows_ok(c) and plan_stem_wgrad(c)["nsplit"] in (6, 2) and plan_stem_wgrad(c)["last"] < plan_stem_wgrad(c)["chunk"],
    "swg.taps_tiles": lambda c: not stem_rows_ok(c) and plan_stem_wgrad(c)["tiles"] in (3, 2) and c.geom[3] % 64 != 0,
    "c4.fwd_narrow": lambda c: c.c == 4 and c.geom[3] < 128 and divmod(c.geom[4] ** 2, 8) == (6, 1),
    "c4.fwd_wide": lambda c: c.c == 4 and c.geom[3] >= 128 and _cdiv(c.geom[4] ** 2, 8) == 2,
    "c4.fwd_stats": lambda c: c.c == 4 and c.geom[3] % 4 == 0,
    "c4.wgrad": lambda c: c.c == 4,
    "stem.refused": lambda c: {"k66": c.geom[3] % 4 != 0, "s9": 3 * c.geom[4] > 24, "ws_short": True, "pmean_only": True}[c.opt["what"]],
    "stem.host": lambda c: c.c == 3 and c.opt["row_stem"] in (0, 1),
}


def documented_branches():
    """{label: selector} from the module docstring's branch table."""
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9]+\.[a-z0-9_]+)\s+((?:conv_mfma\.hip|nn\.py):[A-Za-z_]\w*)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def test_case_table_covers_every_documented_branch():
    """GPU-free: every label of the docstring has a case, every case names only documented labels, every selector the docstring names is defined in the source
    it names, and the selections this file cannot reach are listed as such."""
    doc = documented_branches()
    assert len(doc) == 24, sorted(doc)
    covered = {b for c in CASES for b in c.labels}
    assert not set(doc) - covered, f"documented branches without a case: {sorted(set(doc) - covered)}"
    assert not covered - set(doc), f"cases name undocumented branches: {sorted(covered - set(doc))}"
    assert set(doc) == set(PROPERTY)
    src = _src()
    with open(os.path.join(ROOT, "self-supervised-vision_amd", "nn.py")) as f:
        nn_src = f.read()
    for sel in sorted(set(doc.values())):
        where, name = sel.split(":")
        if where == "nn.py":
            assert re.search(r"^def %s\(" % name, nn_src, re.M), sel
        else:
            assert defines(src, name) or re.search(r"^__device__ [^\n;]*\b%s\(" % name, src, re.M), f"the docstring names {sel}, which the source does not define"
    # the 2^31-byte clauses: documented as unreached, present in both selection functions, and indeed out of every case's reach
    assert set(UNREACHED) == {"sfwd.bytes_2gib", "swg.bytes_2gib"} and not set(UNREACHED) & set(doc)
    assert "Selections this file does not reach" in __doc__
    assert len(re.findall(r"\(int64_t\)d->N \* d->H \* d->W \* 12 < \(1ll << 31\)", src)) == 2
    assert all(c.geom[0] * c.geom[1] * c.geom[2] * 12 < (1 << 31) for c in CASES)
    # every sfwd.taps* case is also the straddle case; every image-stem geometry of the table runs the forward or the weight gradient
    for c in CASES:
        if any(b.startswith("sfwd.taps") for b in c.labels):
            assert "sfwd.taps_straddle" in c.labels, c.id
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert (TAU["fwd"], TAU["wgrad"], TAU["partials"], U, GUARD) == (16.0, 16.0, 16.0, 2.0 ** -24, 1024)


def test_case_shapes_have_the_plan_their_label_claims():
    """GPU-free: the restated selection functions give every case exactly the plan its labels state."""
    q = consts()
    assert (q["SF_ROWS"], q["SF_ROWF"], q["SF_MAXSTEPS"], q["SR_R"], q["SR_ROWF"], q["SR_WO"]) == (9, 728, 77, 7, 728, 112), f"retuned: {q} - re-derive the case table"
    assert (q["SF_PIX_MAX"], q["SF_PIX_MIN"], q["SF_ROUND"], q["SR_ROUND"], q["WG_ROUND"]) == (224, 192, 512, 768, 512), f"retuned: {q} - re-derive the case table"
    for c in CASES:
        for b in c.labels:
            assert PROPERTY[b](c), f"{c.id} does not have the plan that {b} claims: forward {fwd_plan(c) if c.c == 3 else None}, rows {stem_rows_ok(c) and stem_rows_plan(c)}, taps {plan_stem_wgrad(c)}"
    # the two three-digit-N cases stay at the size the table states
    for c in CASES:
        n, h, w, k, r, s, pad = c.geom
        assert n * h * w * 3 <= 1_400_000 and c.m * k <= 7_400_000, c.id


def _lib():
    from ssv_amd import _lib as L
    return L


def _desc(c, arith="f32", n=None):
    L = _lib()
    nn_, h, w, k, r, s, pad = c.geom
    d = L.ConvDesc(nn_ if n is None else n, h, w, c.c, k, r, r, s, pad, c.ho, c.wo)
    if arith == "bf16x3":
        d.arithmetic = L.ARITH_BF16X3
    return d


def test_restatement_agrees_with_the_library_host_side():
    """GPU-free: for every image-stem case the restated selection gives the library's own host-side answers."""
    lib = _lib().load()
    for c in CASES:
        if c.kind != "stem":
            continue
        d = _desc(c)
        fp = fwd_plan(c)
        assert int(lib.ssv_stem_conv_fwd_stats_rows_per_group(C.byref(d))) == fp["group"] == (fp["rpi"] * c.wo if fp["rpi"] else 64), c.id
        assert int(lib.ssv_stem_conv_wgrad_rows_per_group(C.byref(d))) == (stem_rows_plan(c)["rows_per_wg"] if stem_rows_ok(c) else 0), c.id
        assert int(lib.ssv_stem_conv_wgrad_workspace_bytes(C.byref(d))) == wgrad_workspace_bytes(c), c.id
        for product in (0, 2):
            for arith in ("f32", "bf16x3"):
                assert lib.ssv_conv_arithmetic(C.byref(_desc(c, arith)), product) == _lib().ARITH_F32_MFMA, c.id


# ============================================================================================================================ inputs and references
_REF = {}


def _inputs(c):
    """x [N][H][W][C], w [K][R][S][C], dy [N][Ho][Wo][K] on the CPU, drawn once per case id (C == 4: the image's fourth channel is the zero padding)."""
    hit = _REF.setdefault(c.id, {})
    if "x" not in hit:
        n, h, w, k, r, s, pad = c.geom
        g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
        x = torch.randn(n, h, w, c.c, generator=g) + 0.5
        if c.c == 4:
            x[..., 3] = 0.0
        hit["x"] = x
        hit["w"] = torch.randn(k, r, r, c.c, generator=g) * (27 * r * r) ** -0.5
        hit["dy"] = torch.randn(n, c.ho, c.wo, k, generator=g)
    return hit["x"], hit["w"], hit["dy"]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _ref_fwd(c):
    """(ref64, A) of the forward, NHWC, computed once per case."""
    hit = _REF.setdefault(c.id, {})
    if "y64" not in hit:
        x, w, _ = _inputs(c)
        s, pad = c.geom[5], c.geom[6]
        hit["y64"] = F.conv2d(_nchw(x.double()), _nchw(w.double()), stride=s, padding=pad).permute(0, 2, 3, 1).contiguous()
        hit["ya"] = F.conv2d(_nchw(x.double().abs()), _nchw(w.double().abs()), stride=s, padding=pad).permute(0, 2, 3, 1).contiguous()
    return hit["y64"], hit["ya"]


def _ref_wgrad(c):
    """(ref64, A) of the weight gradient as [K][R][S][C], computed once per case."""
    hit = _REF.setdefault(c.id, {})
    if "dw64" not in hit:
        x, w, dy = _inputs(c)
        k, r, s, pad = c.geom[3], c.geom[4], c.geom[5], c.geom[6]
        f = lambda a, b: torch.nn.grad.conv2d_weight(_nchw(a), (k, c.c, r, r), _nchw(b), stride=s, padding=pad).permute(0, 2, 3, 1).contiguous()
        hit["dw64"], hit["dwa"] = f(x.double(), dy.double()), f(x.double().abs(), dy.double().abs())
    return hit["dw64"], hit["dwa"]


def _wrows(c):
    """the filter in the row-taps layout [K][R][24]: 3 S floats of a filter row, zero-padded"""
    _, w, _ = _inputs(c)
    k, r = c.geom[3], c.geom[4]
    out = torch.zeros(k, r, 24)
    out[:, :, :3 * r] = w.reshape(k, r, 3 * r)
    return out


# ============================================================================================================================ GPU helpers
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib().load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_STEM_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


def _out(shape, dev):
    """(buffer, view): an output as a 16-byte aligned view into a NaN-prefilled buffer with GUARD floats of NaN behind it"""
    n = math.prod(shape)
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[:n].view(shape)


def _out_ok(buf, what, written=True):
    n = buf.numel() - GUARD
    if written:
        assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} elements of the output never written (or NaN reached them)"
    assert torch.isnan(buf[n:]).all(), f"{what}: wrote past the end of its buffer"


def _in(t, dev):
    """(buffer, view): an input as a 16-byte aligned view with GUARD floats of NaN in front of it and behind it"""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    buf[GUARD:GUARD + n].copy_(t.reshape(-1))
    view = buf[GUARD:GUARD + n].view(t.shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def _in_ok(buf, t, what):
    n = t.numel()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{what}: the guards around an input were written"
    assert torch.equal(buf[GUARD:GUARD + n].cpu(), t.reshape(-1)), f"{what}: an input changed"


def _record(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


def _bound_check(got, ref, amag, tau, family, what):
    """(a): |got - ref| <= tau * 2^-24 * A + floor (test_gpu_conv_forms._bound_check, with this file's report)."""
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got.double() - ref).abs()
    floor = 1e-30 + 1e-3 * U * float(amag.max())
    bound = tau * U * amag + floor
    ratio = float((err / bound).max())
    print(f"{what}: worst |err| / bound = {ratio:.4f}")
    _record(family, ratio)
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err / bound).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements over the bound; worst at flat {i}: got {float(got.reshape(-1)[i]):.9g} "
                             f"ref {float(ref.reshape(-1)[i]):.9g} A {float(amag.reshape(-1)[i]):.3e} (|err| / bound = {ratio:.2f})")
    return ratio


def _partials_check(pm, p2, y, size, model, family, what):
    """(d): EVERY group of ``size`` rows of y [M][K] (the rows the kernel wrote): mean and centred sum of squares in fp64.  model "first_row": the 64-row
    epilogue that sums around the group's first row (test_gpu_conv_forms._stats_partials' magnitudes); model "two_pass": the rows-in-LDS kernel."""
    m, k = y.shape
    count = _cdiv(m, size)
    assert pm.shape == p2.shape == (count, k), f"{what}: {tuple(pm.shape)} partials for {count} groups"
    y64 = y.double()
    full = m // size
    refs = []
    for blk in ([y64[:full * size].view(full, size, k)] if full else []) + ([y64[full * size:].view(1, m - full * size, k)] if m % size else []):
        mu = blk.mean(1)
        c2 = ((blk - mu[:, None]) ** 2).sum(1)
        if model == "first_row":
            first = blk[:, :1]
            mag_m, mag_2 = first[:, 0].abs() + (blk - first).abs().mean(1), ((blk - first) ** 2).sum(1) * 2
        else:
            mag_m, mag_2 = blk.abs().mean(1), ((blk.abs() + mu.abs()[:, None]) ** 2).sum(1)
        refs.append((mu, c2, mag_m, mag_2))
    mu, c2, mag_m, mag_2 = (torch.cat([r[i] for r in refs]) for i in range(4))
    _bound_check(pm, mu, mag_m, TAU["partials"], family, f"{what} pmean ({count} groups of {size})")
    _bound_check(p2, c2, mag_2, TAU["partials"], family, f"{what} pm2 ({count} groups of {size})")


def _finalize_check(part, y, family, what):
    """ops.bn_stats_finalize on the partials against the fp64 mean / inverse standard deviation of the whole map: the bn-forward rule of
    test_gpu_bn_pool_kernels.py, e(got) <= FACTOR * e(ref32) + FLOOR and the same for m, ref32 = the same lines in float32 on the CPU."""
    from ssv_amd import ops
    m, k = y.shape
    dev_ = y.device
    eps = float(torch.tensor(ops.BN_EPS, dtype=torch.float32))                   # the fp32 value the kernel receives
    gamma, beta = torch.ones(k, device=dev_), torch.zeros(k, device=dev_)
    rm, rv, nbt = torch.zeros(k, device=dev_), torch.ones(k, device=dev_), torch.zeros((), dtype=torch.long, device=dev_)
    mean, invstd, _, _ = ops.bn_stats_finalize(m, k, part, gamma, beta, rm, rv, nbt)
    yc = y.cpu()

    def lines(t):
        mu = t.mean(0)
        var = ((t - mu) ** 2).mean(0)
        return mu, 1.0 / torch.sqrt(var + eps)
    ref64, ref32 = lines(yc.double()), lines(yc)
    for name, got, r64, r32 in (("mean", mean, *[r[0] for r in (ref64, ref32)]), ("invstd", invstd, *[r[1] for r in (ref64, ref32)])):
        g = got.cpu().double()
        assert torch.isfinite(g).all()
        for fig, f in (("e", lambda a: float((a - r64).norm() / r64.norm())), ("m", lambda a: float((a - r64).abs().max() / r64.abs().max()))):
            bar = FACTOR["bn-forward"] * f(r32.double()) + FLOOR["bn-forward"]
            print(f"{what} finalize {name}: {fig}(got) {f(g):.3e}, {fig}(ref32) {f(r32.double()):.3e}, bar {bar:.3e}")
            _record(family, f(g) / bar)
            assert f(g) <= bar, f"{what}: bn_stats_finalize {name}: {fig}(got) {f(g):.3e} over {FACTOR['bn-forward']} * {fig}(ref32) + floor = {bar:.3e}"


def _stem_fwd(c, dev, arith, xv, wr, stats, n=None):
    """One ssv_stem_conv_fwd launch into guarded buffers: (y buffer, y, pmean buffer, pmean, pm2 buffer, pm2)."""
    L = _lib()
    d = _desc(c, arith, n)
    nn_ = d.N
    size = int(L.load().ssv_stem_conv_fwd_stats_rows_per_group(C.byref(d)))
    by, y = _out((nn_, c.ho, c.wo, c.geom[3]), dev)
    bm = pm = b2 = p2 = None
    if stats:
        count = _cdiv(nn_ * c.ho * c.wo, size)
        (bm, pm), (b2, p2) = _out((count, c.geom[3]), dev), _out((count, c.geom[3]), dev)
    L.call("ssv_stem_conv_fwd", C.byref(d), L.ptr(xv), L.ptr(wr), L.ptr(y), L.ptr(pm), L.ptr(p2), L.stream())
    return by, y, bm, pm, b2, p2


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c.id)
def test_stem_forward_against_fp64(dev, case):
    from ssv_amd import ops
    L = _lib()
    lib = L.load()
    c = case
    n, h, w, k, r, s, pad = c.geom
    x, wt, _ = _inputs(c)
    wr_cpu = _wrows(c)
    plan = fwd_plan(c)
    (bx, xv), (bw, wr) = _in(x, dev), _in(wr_cpu, dev)
    size = int(lib.ssv_stem_conv_fwd_stats_rows_per_group(C.byref(_desc(c))))
    assert size == plan["group"], "stem_fwd_rows_rpi as restated in this file is not the library's"
    first = {}
    for arith in ("f32", "bf16x3"):
        with ops.arithmetic(arith):
            for product in (0, 2):
                assert lib.ssv_conv_arithmetic(C.byref(_desc(c, arith)), product) == L.ARITH_F32_MFMA
            by, y, bm, pm, b2, p2 = _stem_fwd(c, dev, arith, xv, wr, True)
            torch.cuda.synchronize()
        what = f"{c.id} [{arith}]"
        for name, buf in (("y", by), ("pmean", bm), ("pm2", b2)):
            _out_ok(buf, f"{what} {name}")                                                     # (e)
        _in_ok(bx, x, what)
        _in_ok(bw, wr_cpu, what)
        if arith == "f32":
            first = dict(y=y, pm=pm, p2=p2)
        else:                                                                                  # (b): the same launch
            assert torch.equal(y, first["y"]) and torch.equal(pm, first["pm"]) and torch.equal(p2, first["p2"]), f"{c.id}: the two arithmetics differ"
    y, pm, p2 = first["y"], first["pm"], first["p2"]
    what = c.id
    # (a)
    ref, amag = (t.to(dev) for t in _ref_fwd(c))
    _bound_check(y, ref, amag, TAU["fwd"], "sfwd.y", f"{what} y")
    if "sfwd.taps_straddle" in c.labels:                                                       # the pixels whose windows start before x / end past it
        assert pad > 0 and plan["kernel"] == "taps"
        _bound_check(y[0, 0, 0], ref[0, 0, 0], amag[0, 0, 0], TAU["fwd"], "sfwd.y", f"{what} y, first pixel of the batch")
        _bound_check(y[-1, -1, -1], ref[-1, -1, -1], amag[-1, -1, -1], TAU["fwd"], "sfwd.y", f"{what} y, last pixel of the batch")
    del ref, amag
    # (d)
    y2 = y.view(c.m, k)
    _partials_check(pm, p2, y2, size, "two_pass" if plan["kernel"] == "rows" else "first_row", "sfwd.partials", what)
    _finalize_check((pm, p2) if size == 64 else (pm, p2, size), y2, "sfwd.finalize", what)
    # (f)
    _, ya, _, pma, _, p2a = _stem_fwd(c, dev, "f32", xv, wr, True)
    assert torch.equal(ya, y) and torch.equal(pma, pm) and torch.equal(p2a, p2), f"{what}: a second identical call differs"
    by0, y0, _, _, _, _ = _stem_fwd(c, dev, "f32", xv, wr, False)
    _out_ok(by0, f"{what} y without statistics")
    assert torch.equal(y0, y), f"{what}: y with statistics != y without"
    del ya, pma, p2a, by0, y0
    wd = wt.permute(0, 3, 1, 2).to(dev)                                                        # [K, 3, R, S] in OHWI memory
    assert ops.can_row_stem(tuple(wd.shape))
    wr_ops = ops.stem_weight_rows(wd)
    assert torch.equal(wr_ops.view(k, r, 24), wr), f"{what}: ops.stem_weight_rows"
    with ops.arithmetic("f32"):
        yo, part = ops.stem_conv_fwd(xv, wr_ops, tuple(wd.shape), s, pad, want_stats=True)
        yn, none = ops.stem_conv_fwd(xv, wr_ops, tuple(wd.shape), s, pad, want_stats=False)
    assert none is None and ops._rows_per_group(part) == size
    assert torch.equal(yo, y) and torch.equal(yn, y) and torch.equal(part[0], pm) and torch.equal(part[1], p2), f"{what}: ops.stem_conv_fwd != the C ABI"
    del yo, yn, part
    per_image = c.ho * c.wo // size if plan["kernel"] == "rows" else 0                         # partials of one image (the 64-row groups cross images)
    for i in sorted({0, n // 2, n - 1}):
        bxi, xi = _in(x[i:i + 1], dev)
        byi, yi, bmi, pmi, b2i, p2i = _stem_fwd(c, dev, "f32", xi, wr, True, n=1)
        for name, buf in ((f"y of image {i} alone", byi), ("its pmean", bmi), ("its pm2", b2i)):
            _out_ok(buf, f"{what} {name}")
        _in_ok(bxi, x[i:i + 1], what)
        assert torch.equal(yi[0], y[i]), f"{what}: y[{i}] of the batch != y of image {i} alone ({int((yi[0] != y[i]).sum())} elements differ)"
        if per_image:
            sl = slice(i * per_image, (i + 1) * per_image)
            assert torch.equal(pmi, pm[sl]) and torch.equal(p2i, p2[sl]), f"{what}: the partials of image {i} alone != its groups in the batch"
    torch.cuda.synchronize()


def _stem_wgrad(c, dev, arith, xv, dyv, short=0):
    L = _lib()
    d = _desc(c, arith)
    k, r = c.geom[3], c.geom[4]
    wsb = int(L.load().ssv_stem_conv_wgrad_workspace_bytes(C.byref(d)))
    assert wsb == wgrad_workspace_bytes(c) and wsb % 4 == 0
    (bd, dwr), (bws, ws) = _out((k, r, 24), dev), _out((wsb // 4,), dev)
    L.call("ssv_stem_conv_wgrad", C.byref(d), L.ptr(xv), L.ptr(dyv), L.ptr(dwr), L.ptr(ws), wsb - short, L.stream())
    return bd, dwr, bws


@pytest.mark.gpu
@pytest.mark.parametrize("case", WG_CASES, ids=lambda c: c.id)
def test_stem_weight_gradient_against_fp64(dev, case):
    from ssv_amd import ops
    L = _lib()
    lib = L.load()
    c = case
    n, h, w, k, r, s, pad = c.geom
    x, _, dy = _inputs(c)
    (bx, xv), (bdy, dyv) = _in(x, dev), _in(dy, dev)
    assert int(lib.ssv_stem_conv_wgrad_rows_per_group(C.byref(_desc(c)))) == (stem_rows_plan(c)["rows_per_wg"] if stem_rows_ok(c) else 0)
    first = None
    for arith in ("f32", "bf16x3"):
        with ops.arithmetic(arith):
            assert lib.ssv_conv_arithmetic(C.byref(_desc(c, arith)), 2) == L.ARITH_F32_MFMA
            bd, dwr, bws = _stem_wgrad(c, dev, arith, xv, dyv)
            torch.cuda.synchronize()
        what = f"{c.id} [{arith}]"
        _out_ok(bd, f"{what} dwrows")                                                          # (e)
        _out_ok(bws, f"{what} workspace", written=False)
        _in_ok(bx, x, what)
        _in_ok(bdy, dy, what)
        assert (dwr[:, :, 3 * r:] == 0).all(), f"{what}: the padding columns e >= 3 S of dwrows are not exact zeros"
        if first is None:
            first = dwr
        else:
            assert torch.equal(dwr, first), f"{c.id}: the two arithmetics differ"
    dwr, what = first, c.id
    ref, amag = _ref_wgrad(c)
    full, fmag = torch.zeros(k, r, 24, dtype=torch.float64), torch.zeros(k, r, 24, dtype=torch.float64)
    full[:, :, :3 * r], fmag[:, :, :3 * r] = ref.reshape(k, r, 3 * r), amag.reshape(k, r, 3 * r)
    _bound_check(dwr, full.to(dev), fmag.to(dev), TAU["wgrad"], "swg.dwrows", f"{what} dwrows")  # (a): all K R 24 entries
    _, again, _ = _stem_wgrad(c, dev, "f32", xv, dyv)                                          # (f)
    assert torch.equal(again, dwr), f"{what}: a second identical call differs"
    with ops.arithmetic("f32"):
        via_ops = ops.stem_conv_wgrad(xv, dyv, (k, 3, r, r), s, pad)
    assert via_ops.shape == (k * r, 24) and torch.equal(via_ops.view(k, r, 24), dwr), f"{what}: ops.stem_conv_wgrad != the C ABI"
    torch.cuda.synchronize()


# ============================================================================================================================ the image padded to 4 channels
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "c4"], ids=lambda c: c.id)
def test_padded_stem_forward_against_fp64(dev, case):
    from ssv_amd import ops
    L = _lib()
    lib = L.load()
    c = case
    n, h, w, k, r, s, pad = c.geom
    x, wt, _ = _inputs(c)
    (bx, xv), (bw, wv) = _in(x, dev), _in(wt, dev)
    groups = int(lib.ssv_conv2d_fwd_stats_groups(C.byref(_desc(c))))
    assert groups == _cdiv(c.m, 64)
    outs = {}
    for arith in ("f32", "bf16x3"):
        d = _desc(c, arith)
        with ops.arithmetic(arith):
            assert lib.ssv_conv_arithmetic(C.byref(d), 0) == L.ARITH_F32_MFMA
            for rep in (0, 1):
                (by, y), (bm, pm), (b2, p2), (bp, yp) = _out((n, c.ho, c.wo, k), dev), _out((groups, k), dev), _out((groups, k), dev), _out((n, c.ho, c.wo, k), dev)
                L.call("ssv_conv2d_fwd_stats", C.byref(d), L.ptr(xv), L.ptr(wv), L.ptr(y), L.ptr(pm), L.ptr(p2), L.stream())
                L.call("ssv_conv2d_fwd", C.byref(d), L.ptr(xv), L.ptr(wv), None, None, L.ptr(yp), L.stream())
                torch.cuda.synchronize()
                what = f"{c.id} [{arith}]"
                for name, buf in (("y", by), ("pmean", bm), ("pm2", b2), ("y (ssv_conv2d_fwd)", bp)):
                    _out_ok(buf, f"{what} {name}")
                _in_ok(bx, x, what)
                _in_ok(bw, wt, what)
                assert torch.equal(y, yp), f"{what}: y with statistics != y without"
                outs.setdefault("first", (y, pm, p2))
                assert all(torch.equal(a, b) for a, b in zip(outs["first"], (y, pm, p2))), f"{what}: a second call, or the other arithmetic, differs"
    y, pm, p2 = outs["first"]
    ref, amag = (t.to(dev) for t in _ref_fwd(c))
    _bound_check(y, ref, amag, TAU["fwd"], "c4.y", f"{c.id} y")
    y2 = y.view(c.m, k)
    _partials_check(pm, p2, y2, 64, "first_row", "c4.partials", c.id)
    _finalize_check((pm, p2), y2, "c4.finalize", c.id)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "c4wgrad"], ids=lambda c: c.id)
def test_padded_stem_weight_gradient_against_fp64(dev, case):
    from ssv_amd import ops
    L = _lib()
    lib = L.load()
    c = case
    n, h, w, k, r, s, pad = c.geom
    x, _, dy = _inputs(c)
    (bx, xv), (bdy, dyv) = _in(x, dev), _in(dy, dev)
    ref, amag = (t.to(dev) for t in _ref_wgrad(c))
    rel = {}
    for arith in ("f32", "bf16x3"):
        d = _desc(c, arith)
        with ops.arithmetic(arith):
            used = lib.ssv_conv_arithmetic(C.byref(d), 2)
            assert used == (L.ARITH_BF16X3 if arith == "bf16x3" else L.ARITH_F32_MFMA)           # C % 4 == 0 and K % 4 == 0: the one-accumulator form
            wsb = int(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d)))
            got = []
            for rep in (0, 1):
                (bd, dw), (bws, ws) = _out((k, r, r, 4), dev), _out((wsb // 4 + 1,), dev)
                L.call("ssv_conv2d_wgrad", C.byref(d), L.ptr(xv), L.ptr(dyv), L.ptr(dw), 0, L.ptr(ws), wsb, L.stream())
                torch.cuda.synchronize()
                what = f"{c.id} [{arith}]"
                _out_ok(bd, f"{what} dw")
                _out_ok(bws, f"{what} workspace", written=False)
                _in_ok(bx, x, what)
                _in_ok(bdy, dy, what)
                got.append(dw)
        assert torch.equal(got[0], got[1]), f"{what}: a second identical call differs"
        assert (got[0][..., 3] == 0).all(), f"{what}: the padded input channel's column is not exactly zero"
        _bound_check(got[0], ref, amag, TAU["wgrad"], "c4.dw", f"{what} dw")
        rel[arith] = float((got[0].double() - ref).norm() / ref.norm())
    assert rel["bf16x3"] <= 1.05 * rel["f32"] + 1e-9, f"{c.id}: bf16x3 {rel['bf16x3']:.3e} vs fp32 MFMA {rel['f32']:.3e} against fp64"


# ============================================================================================================================ refusals
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "refused"], ids=lambda c: c.id)
def test_refused_stem_launches_leave_their_outputs_alone(dev, case):
    L = _lib()
    lib = L.load()
    c = case
    n, h, w, k, r, s, pad = c.geom
    what = c.opt["what"]
    x, _, dy = _inputs(c)
    (bx, xv), (bdy, dyv) = _in(x, dev), _in(dy, dev)
    _, wr = _in(torch.zeros(k, r, 24), dev)
    d = _desc(c)
    P = L.ptr
    (by, y), (bm, pm), (b2, p2), (bd, dwr) = _out((n, c.ho, c.wo, k), dev), _out((c.m, k), dev), _out((c.m, k), dev), _out((k, r, 24), dev)
    wsb = int(lib.ssv_stem_conv_wgrad_workspace_bytes(C.byref(d)))
    bws, ws = _out((wsb // 4 + 4,), dev)

    def refused(rc, who):
        msg = lib.ssv_last_error().decode()
        assert rc != 0, f"{c.id}: {who} accepted the launch"
        assert who in msg and len(msg) > len(who) + 4, f"{c.id}: {who} returned {rc} with the message {msg!r}"
    if what in ("k66", "s9", "pmean_only"):
        refused(lib.ssv_stem_conv_fwd(C.byref(d), P(xv), P(wr), P(y), P(pm), None if what == "pmean_only" else P(p2), L.stream()), "ssv_stem_conv_fwd")
    if what in ("k66", "s9", "ws_short"):
        refused(lib.ssv_stem_conv_wgrad(C.byref(d), P(xv), P(dyv), P(dwr), P(ws), wsb - 1 if what == "ws_short" else wsb, L.stream()), "ssv_stem_conv_wgrad")
    torch.cuda.synchronize()
    for name, buf in (("y", by), ("pmean", bm), ("pm2", b2), ("dwrows", bd), ("workspace", bws)):
        assert torch.isnan(buf).all(), f"{c.id}: a refused call wrote {name}"
    _in_ok(bx, x, c.id)
    _in_ok(bdy, dy, c.id)


# ============================================================================================================================ nn.stem_conv with a tape
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "host"], ids=lambda c: c.id)
def test_nn_stem_conv_with_a_tape_against_fp64(dev, case):
    from ssv_amd import nn as hnn
    from ssv_amd import ops
    c = case
    n, h, w, k, r, s, pad = c.geom
    x, wt, dy = _inputs(c)
    g = torch.Generator().manual_seed(zlib.crc32((c.id + "/prior").encode()))
    prior = torch.randn(k, r, r, 3, generator=g)
    (bx, xv), (bdy, dyv) = _in(x, dev), _in(dy, dev)
    weight = torch.nn.Parameter(wt.to(dev).permute(0, 3, 1, 2))                                # [K, 3, R, S], OHWI memory
    weight.grad = prior.to(dev).permute(0, 3, 1, 2)
    prev = hnn._ROW_STEM, hnn._FUSE_BN_STATS
    hnn._ROW_STEM, hnn._FUSE_BN_STATS = bool(c.opt["row_stem"]), True
    try:
        tape = hnn.Tape(xv, False)
        y = hnn.stem_conv(tape, xv, weight, s, pad, bn_stats=True)
        part = y._bn_partials
        assert len(tape.ops) == 1
        assert tape.backward(y, dyv) is None                                                   # images take no gradient
        torch.cuda.synchronize()
    finally:
        hnn._ROW_STEM, hnn._FUSE_BN_STATS = prev
    _in_ok(bx, x, c.id)
    _in_ok(bdy, dy, c.id)
    size = ops._rows_per_group(part)
    assert size == (fwd_plan(c)["group"] if c.opt["row_stem"] else 64)
    ref, amag = (t.to(dev) for t in _ref_fwd(c))
    _bound_check(y, ref, amag, TAU["fwd"], "host.y", f"{c.id} y")
    y2 = y.view(c.m, k)
    _partials_check(part[0], part[1], y2, size, "two_pass" if fwd_plan(c)["kernel"] == "rows" and c.opt["row_stem"] else "first_row", "host.partials", c.id)
    _finalize_check(part, y2, "host.finalize", c.id)
    dref, dmag = _ref_wgrad(c)
    got = weight.grad.permute(0, 2, 3, 1)
    _bound_check(got, (prior.double() + dref).to(dev), (prior.double().abs() + dmag).to(dev), TAU["wgrad"], "host.dw", f"{c.id} prior + dW")
