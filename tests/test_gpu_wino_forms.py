"""Every Winograd transform and batched-GEMM launch (csrc/winograd.hip, csrc/winograd44.hip and the ssv_gemm_batched* entry points at the end of
csrc/conv_mfma.hip), ONE STAGE AT A TIME, against the float64 restatement of the same stage (tests/wino_oracle.py, proven GPU-free by
tests/test_wino_oracle_cpu.py).  tests/test_gpu_winograd.py, test_gpu_winograd44.py and test_gpu_split.py run the whole chain through ops.*; this file calls
every C-ABI entry point on its own, straight through _lib.call.

Each case of CASES names the entry points it calls, the branch labels it reaches and its geometry (all maps <= 12 x 12, N <= 5).  The inputs are drawn on the CPU
from a generator seeded by the case id, so the GPU-free tests see what the GPU tests upload.  Every run is held to:

  (a) accuracy of the stage alone: ref64 = the oracle in float64, ref32 = the SAME lines in float32, e(x) = ||x - ref64||_2 / ||ref64||_2 and
      m(x) = max|x - ref64| / max|ref64|:   e(got) <= FACTOR[family] * e(ref32) + FLOOR   and the same for m.  The exact stages - F(2x2)'s input and dY
      transforms (adds only), its filter transform, filter gradient and output transform (adds and halves; the oracle is written in the kernels' order of
      operations), gated or not - are bit-identical to ref32.  The GEMM stages keep the bounds of tests/test_gpu_conv_forms.py: element-wise
      |got - ref64| <= 16 * 2^-24 * (|a| . |b|) + floor in both arithmetics, and the bf16x3 relative l2 error <= 1.05 x the fp32-MFMA one + 1e-9;
  (b) test_reference_is_well_conditioned, GPU-free: ref64 finite and not identically zero, ref32 within 1e-3 of it (e and m);
  (c) partials group by group: every row of pmean / pm2 and psum_g / psum_gx against the float64 value over exactly the rows the kernel headers give that
      group (wino_oracle.group_rows) of the y the kernel wrote - the short last group of F(2x2) included - under (a)'s bar row by row; the group count is
      the library's answer and nothing behind that many rows is written;
  (d) every output and workspace is a 16-byte aligned view into a NaN-prefilled buffer with 1024 floats of guard behind an output and 4096 behind a
      workspace: no element of an output stays NaN (all 16 / 36 positions of every tile of V, dM and Vd on ragged maps, every pixel of y), the guard is
      untouched, every input is bit-identical afterwards;
  (e) the bitwise identities the sources state: ssv_wino44_dy_transform_both(dyin NULL) == ssv_wino44_input_transform(dy) and ssv_wino44_dy_transform(dy),
      with dyin == (under (a)) the two transforms of the formed dy; V2 of ssv_wino44_input_transform == ssv_wino_input_transform's output and V the same bits
      with and without V2; the fused input == the transform of what ssv_bn_apply (relu) materialises; the byte-mask gate == the scale + shift gate (y and
      partials; the mask is the float64 sign, which is the sign of the kernel's fmaf); filter_grad accumulating on a zero prior == overwriting, on a seeded
      prior == prior + overwrite within one rounding; a second identical call == the first;
  (f) refusals (REFUSALS) return a non-zero status, set ssv_last_error and leave their outputs NaN.

FACTOR and FLOOR follow the rule of tests/test_gpu_bn_pool_kernels.py: FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured
per family on an MI355X (profiles/wino_forms_report.json, written by this file under SSV_WINO_REPORT=<path>), rounded up to the next power of two and never
above 8; FLOOR = 2 * 2^-24 for outputs ref32 gets exactly.

The lane mapping of the two output transforms (lane_plan) and plan_batched_wgrad / wgrad_row_split of conv_mfma.hip (wgrad_plan) are restated below;
test_case_shapes_have_the_property_their_label_claims holds every case to the property its label names.

Branch labels (label, entry points, what the case reaches) - test_case_table_covers_every_documented_branch keeps CASES honest:

  lanes.lt16           ssv_wino_output_transform        K < 64: TPP = 256 / (K / 4) > 16 tiles of a group, at least two groups (the lanes past the group idle)
  lanes.tpp            ssv_wino_output_transform        K 128, 256 (F(4x4): L < 256 too): the LDS merge of several tiles per channel lane
  lanes.one            ssv_wino_output_transform        L = 256, TPP 1: K 1024 (F(2x2)), 512 (F(4x4))
  lanes.gy2            ssv_wino_output_transform        blockIdx.y > 0: K 2048 (F(2x2)), 1024 (F(4x4))
  lanes.k4             ssv_wino44_output_transform      K 4: L 2, TPP 128 > the tiles of a group
  map.whole            ssv_wino_input_transform         H and W multiples of the tile
  map.ragged_h         ssv_wino_input_transform         H no multiple of the tile
  map.ragged_w         ssv_wino_input_transform         W no multiple of the tile
  map.sub_tile         ssv_wino_input_transform         H or W smaller than the tile
  stats.rowgroups      ssv_wino44_output_transform      H % 4 == 0: one partial per row of tiles (4 W rows)
  stats.image          ssv_wino44_output_transform      H % 4 != 0: one partial per image
  stats.g64            ssv_wino_output_transform        even map: 64 rows per partial
  stats.image16        ssv_wino_output_transform        7 x 7: one image = 16 tiles = one partial of 49 rows
  stats.short_last     ssv_wino_output_transform        T % 16 != 0: the last partial is short
  gate.affine          ssv_wino_output_transform        ReLU bit recomputed from x * scale + shift (ragged maps: F(4x4)'s clamped loads must not reach the sums)
  gate.mask            ssv_wino_output_transform        ReLU bit from the byte mask
  in.plain             ssv_wino_input_transform         x as it is; C 4 and 36 (no % 32 here)
  in.xf                ssv_wino_input_transform         relu(x * scale + shift) formed on load
  in.v2                ssv_wino44_input_transform       the F(2x2) operand beside F(4x4)'s own (2 channels per thread)
  in.xf_v2             ssv_wino44_input_transform       both
  dy.plain             ssv_wino_dy_transform            A dY A^T; K 4, 36, 128
  dy.both              ssv_wino44_dy_transform_both     Vd and dM from one pass
  dy.both_dyin         ssv_wino44_dy_transform_both     ... of the output gradient formed on load
  filt.fwd             ssv_wino_filter_transform        K * C no multiple of 256; C 3
  filt.grad_acc0       ssv_wino_filter_grad             overwrite
  filt.grad_acc1       ssv_wino_filter_grad             accumulate on a zero and on a seeded prior
  gemm.f32             ssv_gemm_batched                 batch 16 and 36, ragged rows (27, 130), K 64 / 132 / 260
  gemm.sp1             ssv_gemm_batched_split           C <= 1152: one accumulator; addend in place, bias at batch 1
  gemm.sp2             ssv_gemm_batched_split           C 1184: two accumulators
  wgrad.tile.64x64     ssv_gemm_batched_wgrad           K < 128, C <= 64 (C 36: ragged tile columns)
  wgrad.tile.128x64    ssv_gemm_batched_wgrad           K >= 128 (132: ragged), C <= 64
  wgrad.tile.64x128    ssv_gemm_batched_wgrad           K < 128, C > 64
  wgrad.tile.128x128   ssv_gemm_batched_wgrad           K >= 128, C > 64
  wgrad.chunked        ssv_gemm_batched_wgrad_blocked   max_chunk_rows 32 and 64 on 300 rows
  wgrad.flushed        ssv_gemm_batched_wgrad_blocked   flush 128 on 27, 128, 129, 300 rows
  wgrad.both           ssv_gemm_batched_wgrad_blocked   chunk and flush
  wgrad.nsplit_lt4     ssv_gemm_batched_wgrad_blocked   1, 2 and 3 slabs: the empty row groups of the float64 fold

Measured on an MI355X (profiles/wino_forms_report.json): see FACTOR below and DESIGN.md section 2.
"""
import ctypes as C
import json
import math
import os
import re
import zlib

import pytest
import torch

import wino_oracle as wo

U = 2.0 ** -24
GUARD, WS_GUARD = 1024, 4096                                             # floats of NaN behind every output / workspace
# one pair per family, by the rule of the docstring from the MI355X run committed as profiles/wino_forms_report.json.  Measured worst ratios: f22 2.45 (psum_gx
# of the gated output at K = 8 on the 9 x 5 map; every transformed tensor and y of F(2x2) but the fused input is bit-exact, the fused input 0.50), f44 7.54 (pmean
# at K = 1024 on the 7 x 12 map, one image of 84 rows per thread: wino44_output_k sums about the thread's first pixel, and on a channel whose first pixel is an
# outlier the running sum loses a digit; 4.83 on 12 x 12 x 512; the transforms themselves stay below 1.0 and its y below 0.6).  wino_output_k measured 16 on
# 8 x 8 x 1024 with the same sums and now merges tile by tile (0.91).  The products: worst |err| / bound 0.32, bf16x3 at most 0.75 x the fp32-MFMA error.
FACTOR = {"f22": 4.0, "f44": 8.0}
FLOOR = 2 * U
COND = 1e-3
GEMM_TAU, GEMM_BF16_BAR = 16.0, 1.05                                     # tests/test_gpu_conv_forms.py's bounds
REPORT, WORST = {}, {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F22, F44 = wo.F22, wo.F44
FAMKEY = {F22: "f22", F44: "f44"}
PFX = {F22: "ssv_wino_", F44: "ssv_wino44_"}


def _fmt(v):
    if isinstance(v, bool):
        return "y" if v else "n"
    if isinstance(v, (tuple, list)):
        return "x".join(_fmt(a) for a in v)
    return str(v)


class Case:
    def __init__(self, kind, entries, labels, **p):
        self.kind, self.entries, self.labels, self.p = kind, tuple(entries.split()), tuple(labels.split()), p
        self.id = kind + "".join(f"-{k}{_fmt(v)}" for k, v in p.items())

    def __getitem__(self, k):
        return self.p.get(k)

    def gen(self):
        return torch.Generator().manual_seed(zlib.crc32(self.id.encode()))


# ====================================================================================================================== the plans, restated
def lane_plan(fam, k):
    """wino_output_k (4 channels per thread) / wino44_output_k (2): lanes along the channels, tiles per pass, y-blocks"""
    kv = k // (4 if fam == F22 else 2)
    lanes = min(kv, 256)
    return {"L": lanes, "TPP": 256 // lanes, "GY": wo.cdiv(kv, 256)}


def wgrad_plan(batch, rows, c, k, max_chunk=0):
    """plan_batched_wgrad + wgrad_row_split of conv_mfma.hip"""
    bm, bn = (128 if k >= 128 else 64), (64 if c <= 64 else 128)
    tiles = wo.cdiv(k, bm) * wo.cdiv(c, bn)
    ns = max(1, min((768 if bm == 128 else 1024) // (tiles * batch), wo.cdiv(rows, 256)))
    chunk = wo.cdiv(wo.cdiv(rows, ns), 32) * 32
    if max_chunk > 0 and chunk > max_chunk:
        chunk = wo.cdiv(wo.cdiv(rows, wo.cdiv(rows, max_chunk)), 32) * 32
    return {"bm": bm, "bn": bn, "nsplit": wo.cdiv(rows, chunk), "chunk": chunk}


def map_labels(t, h, w):
    out = []
    if h % t == 0 and w % t == 0:
        out.append("map.whole")
    if h % t:
        out.append("map.ragged_h")
    if w % t:
        out.append("map.ragged_w")
    if h < t or w < t:
        out.append("map.sub_tile")
    return " ".join(out)


# ====================================================================================================================== the table
def _filt(k, c):
    return Case("filt", "ssv_wino_filter_transform ssv_wino_filter_grad ssv_wino44_filter_transform ssv_wino44_filter_grad",
                "filt.fwd filt.grad_acc0 filt.grad_acc1", K=k, C=c)


def _in(n, h, w, c):
    return Case("in", "ssv_wino_input_transform ssv_wino44_input_transform", "in.plain in.xf in.v2 in.xf_v2 " + map_labels(4, h, w), N=n, H=h, W=w, C=c)


def _dy(n, h, w, k):
    return Case("dy", "ssv_wino_dy_transform ssv_wino44_dy_transform ssv_wino44_dy_transform_both", "dy.plain dy.both dy.both_dyin " + map_labels(4, h, w),
                N=n, H=h, W=w, K=k)


def _out(fam, mode, n, h, w, k, labels):
    return Case("out", PFX[fam] + "output_transform", labels + " " + map_labels(wo.TILE[fam], h, w) + (" gate.affine gate.mask" if mode == "gate" else ""),
                fam=fam, mode=mode, N=n, H=h, W=w, K=k)


def _gemm(batch, rows, c, k, form, addend=False, bias=False):
    return Case("gemm", "ssv_gemm_batched ssv_gemm_batched_split", "gemm.f32 gemm." + form, batch=batch, rows=rows, C=c, K=k, addend=addend, bias=bias)


def _wgrad(batch, rows, c, k, labels, chunk=0, flush=0):
    entry = "ssv_gemm_batched_wgrad_blocked ssv_gemm_batched_wgrad_blocked_workspace_bytes" if (chunk or flush) else "ssv_gemm_batched_wgrad ssv_gemm_batched_wgrad_workspace_bytes"
    return Case("wgrad", entry + " ssv_gemm_batched_wgrad_split", labels, batch=batch, rows=rows, C=c, K=k, chunk=chunk, flush=flush)


CASES = [
    _filt(12, 20), _filt(7, 3), _filt(36, 8),
    _in(2, 8, 8, 4), _in(2, 7, 8, 36), _in(3, 8, 6, 4), _in(2, 9, 5, 36), _in(5, 3, 2, 4), _in(1, 12, 12, 36), _in(3, 7, 7, 4),
    _dy(2, 8, 8, 4), _dy(2, 7, 8, 36), _dy(2, 8, 6, 128), _dy(3, 9, 5, 4), _dy(5, 3, 2, 36), _dy(3, 7, 7, 128),
    # ---- F(2x2) output transform
    _out(F22, "plain", 2, 8, 8, 32, "lanes.lt16"), _out(F22, "stats", 2, 8, 8, 32, "lanes.lt16 stats.g64"), _out(F22, "gate", 2, 8, 8, 32, "lanes.lt16"),
    _out(F22, "stats", 3, 7, 7, 32, "lanes.lt16 stats.image16"), _out(F22, "gate", 3, 7, 7, 4, "lanes.lt16"), _out(F22, "stats", 3, 8, 8, 16, "lanes.lt16 stats.g64"),
    _out(F22, "gate", 3, 9, 5, 8, "lanes.lt16"),
    _out(F22, "stats", 2, 8, 6, 128, "lanes.tpp stats.g64 stats.short_last"), _out(F22, "gate", 1, 8, 8, 256, "lanes.tpp"), _out(F22, "gate", 3, 9, 5, 128, "lanes.tpp"),
    _out(F22, "plain", 3, 9, 5, 128, "lanes.tpp"), _out(F22, "stats", 2, 7, 7, 256, "lanes.tpp stats.image16"),
    _out(F22, "stats", 1, 8, 8, 1024, "lanes.one stats.g64"), _out(F22, "gate", 1, 7, 8, 1024, "lanes.one"),
    _out(F22, "plain", 1, 4, 4, 2048, "lanes.gy2"), _out(F22, "gate", 1, 4, 6, 2048, "lanes.gy2"), _out(F22, "stats", 1, 4, 6, 2048, "lanes.gy2 stats.g64 stats.short_last"),
    _out(F22, "plain", 5, 3, 1, 128, "lanes.tpp"),
    # ---- F(4x4) output transform
    _out(F44, "stats", 2, 8, 8, 4, "lanes.k4 stats.rowgroups"), _out(F44, "gate", 2, 8, 8, 4, "lanes.k4"), _out(F44, "gate", 3, 9, 5, 4, "lanes.k4"),
    _out(F44, "stats", 2, 7, 6, 128, "lanes.tpp stats.image"), _out(F44, "stats", 2, 6, 5, 256, "lanes.tpp stats.image"), _out(F44, "gate", 2, 6, 5, 256, "lanes.tpp"),
    _out(F44, "stats", 5, 12, 12, 128, "lanes.tpp stats.rowgroups"), _out(F44, "plain", 2, 7, 8, 128, "lanes.tpp"),
    _out(F44, "stats", 2, 8, 8, 512, "lanes.one stats.rowgroups"), _out(F44, "stats", 1, 12, 12, 512, "lanes.one stats.rowgroups"),
    _out(F44, "stats", 2, 7, 12, 1024, "lanes.gy2 stats.image"), _out(F44, "gate", 2, 9, 5, 512, "lanes.one"),
    _out(F44, "gate", 1, 4, 4, 1024, "lanes.gy2"), _out(F44, "stats", 1, 8, 6, 1024, "lanes.gy2 stats.rowgroups"),
    _out(F44, "plain", 3, 3, 2, 128, "lanes.tpp"), _out(F44, "gate", 3, 3, 2, 128, "lanes.tpp"),
    # ---- the batched products
    _gemm(16, 27, 64, 64, "sp1"), _gemm(36, 130, 128, 132, "sp1", addend=True), _gemm(16, 27, 1184, 260, "sp2"), _gemm(1, 130, 64, 260, "sp1", addend=True, bias=True),
    _gemm(36, 27, 1184, 64, "sp2", addend=True),
    _wgrad(16, 300, 36, 64, "wgrad.tile.64x64"), _wgrad(36, 130, 36, 132, "wgrad.tile.128x64"), _wgrad(16, 27, 128, 64, "wgrad.tile.64x128"),
    _wgrad(16, 130, 132, 132, "wgrad.tile.128x128"),
    _wgrad(16, 300, 36, 132, "wgrad.chunked wgrad.tile.128x64", chunk=32), _wgrad(36, 300, 128, 64, "wgrad.chunked wgrad.tile.64x128", chunk=64),
    _wgrad(16, 27, 36, 64, "wgrad.flushed wgrad.nsplit_lt4 wgrad.tile.64x64", flush=128), _wgrad(16, 128, 36, 64, "wgrad.flushed wgrad.nsplit_lt4 wgrad.tile.64x64", flush=128),
    _wgrad(36, 129, 132, 132, "wgrad.flushed wgrad.nsplit_lt4 wgrad.tile.128x128", flush=128), _wgrad(16, 300, 36, 64, "wgrad.flushed wgrad.nsplit_lt4 wgrad.tile.64x64", flush=128),
    _wgrad(16, 600, 36, 64, "wgrad.flushed wgrad.nsplit_lt4 wgrad.tile.64x64", flush=128),
    _wgrad(16, 300, 36, 132, "wgrad.both wgrad.tile.128x64", chunk=64, flush=128), _wgrad(36, 300, 128, 132, "wgrad.both wgrad.tile.128x128", chunk=128, flush=128),
]


def header_entry_points():
    """every ssv_wino_*, ssv_wino44_* and ssv_gemm_batched* function include/ssv_hip.h declares"""
    src = open(os.path.join(ROOT, "include", "ssv_hip.h")).read()
    return set(re.findall(r"^(?:int|int32_t|int64_t|size_t)\s+(ssv_(?:wino_|wino44_|gemm_batched)\w*)\(", src, re.M))


HOST_ANSWERS = {"ssv_wino_tiles", "ssv_wino_groups", "ssv_wino_stats_rows_per_group", "ssv_wino44_tiles", "ssv_wino44_groups", "ssv_wino44_stats_rows_per_group"}


def documented_branches():
    return {m.group(1): m.group(2) for m in (re.match(r"^  ([a-z0-9_]+\.[a-z0-9_.]+)\s+(ssv_\w+)\s", ln) for ln in __doc__.splitlines()) if m}


def test_case_table_names_every_entry_point():
    """GPU-free: every Winograd and batched-GEMM symbol of the header is called by a case (the six host answers: by every `out` / `in` / `dy` run, and GPU-free by
    tests/test_wino_oracle_cpu.py), and every name a case gives is a symbol of the header."""
    hdr = header_entry_points()
    assert len(hdr) == 24 and HOST_ANSWERS <= hdr, sorted(hdr)
    named = {e for c in CASES for e in c.entries}
    assert not named - hdr, f"cases name symbols the header does not declare: {sorted(named - hdr)}"
    missing = hdr - HOST_ANSWERS - named
    assert not missing, f"entry points without a case: {sorted(missing)}"
    from ssv_amd import _lib
    assert hdr <= set(_lib.SIGNATURES)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_case_table_covers_every_documented_branch():
    """GPU-free: every label of the docstring has a case (the labels both output transforms share: one per family), every label of a case is documented,
    and the entry point the docstring names beside a label is one the header declares."""
    doc = documented_branches()
    assert len(doc) == 37, sorted(doc)
    covered = {b for c in CASES for b in c.labels}
    assert not set(doc) - covered, f"documented branches without a case: {sorted(set(doc) - covered)}"
    assert not covered - set(doc), f"cases name undocumented branches: {sorted(covered - set(doc))}"
    assert set(doc.values()) <= header_entry_points()
    for lab in ("lanes.tpp", "lanes.one", "lanes.gy2", "gate.affine", "gate.mask", "map.whole", "map.ragged_h", "map.ragged_w", "map.sub_tile"):
        for fam in (F22, F44):
            assert any(lab in c.labels and (c["fam"] == fam or c.kind in ("in", "dy")) for c in CASES), f"{lab}: no case of family {fam}"
    for mode in ("plain", "stats", "gate"):
        assert any(c.kind == "out" and c["fam"] == F22 and c["mode"] == mode and "lanes.lt16" in c.labels for c in CASES), mode


def test_case_shapes_have_the_property_their_label_claims():
    """GPU-free: a retuned lane mapping or weight-gradient plan fails here instead of hollowing the table out"""
    for c in CASES:
        lab = set(c.labels)
        if c["H"] is not None:
            n, h, w = c["N"], c["H"], c["W"]
            assert h <= 12 and w <= 12 and n <= 5, c.id
            t = wo.TILE[c["fam"]] if c.kind == "out" else 4
            assert set(map_labels(t, h, w).split()) == {x for x in lab if x.startswith("map.")}, c.id
        if c.kind == "out":
            fam, k, mode = c["fam"], c["K"], c["mode"]
            p = lane_plan(fam, k)
            tiles, groups = wo.tiles(fam, n, h, w), wo.groups(fam, n, h, w, mode == "stats")
            gtiles = 16 if fam == F22 else tiles // groups
            assert ("lanes.lt16" in lab) == (fam == F22 and k < 64), c.id
            if "lanes.lt16" in lab:
                assert p["TPP"] > 16 and tiles >= 32 and groups >= 2, c.id
            if "lanes.k4" in lab:
                assert fam == F44 and k == 4 and p["L"] == 2 and p["TPP"] == 128 > gtiles, c.id
            if "lanes.tpp" in lab:
                assert 1 < p["TPP"] <= 16 and p["GY"] == 1, c.id
            if "lanes.one" in lab:
                assert p["L"] == 256 and p["TPP"] == 1 and p["GY"] == 1, c.id
            if "lanes.gy2" in lab:
                assert p["GY"] == 2, c.id
            assert len([x for x in lab if x.startswith("lanes.")]) == 1, c.id
            if mode == "stats":
                rpg = wo.stats_rows_per_group(fam, n, h, w)
                assert rpg > 0, c.id
                want = set()
                if fam == F44:
                    want.add("stats.rowgroups" if h % 4 == 0 else "stats.image")
                    assert (rpg == 4 * w and groups == n * h // 4) if h % 4 == 0 else (rpg == h * w and groups == n), c.id
                else:
                    want.add("stats.g64" if h % 2 == 0 and w % 2 == 0 else "stats.image16")
                    assert rpg == (64 if "stats.g64" in want else h * w) and ("stats.g64" in want or tiles // n == 16), c.id
                    if tiles % 16:
                        want.add("stats.short_last")
                assert want == {x for x in lab if x.startswith("stats.")}, c.id
            else:
                assert not any(x.startswith("stats.") for x in lab), c.id
            assert (mode == "gate") == ("gate.affine" in lab) == ("gate.mask" in lab), c.id
        if c.kind in ("in", "dy"):
            assert (c["C"] or c["K"]) in (4, 36, 128), c.id
        if c.kind == "filt":
            assert (c["K"] * c["C"]) % 256 != 0, c.id
        if c.kind == "gemm":
            assert c["batch"] in (1, 16, 36) and c["C"] % 32 == 0 and c["K"] % 4 == 0, c.id
            assert ("gemm.sp2" in lab) == (c["C"] > 1152) and ("gemm.sp1" in lab) == (c["C"] <= 1152), c.id
            assert not c["bias"] or c["batch"] == 1, c.id
        if c.kind == "wgrad":
            p = wgrad_plan(c["batch"], c["rows"], c["C"], c["K"], c["chunk"])
            assert f"wgrad.tile.{p['bm']}x{p['bn']}" in lab and len([x for x in lab if x.startswith("wgrad.tile.")]) == 1, c.id
            assert ("wgrad.chunked" in lab) == (c["chunk"] > 0 and c["flush"] == 0), c.id
            assert ("wgrad.flushed" in lab) == (c["chunk"] == 0 and c["flush"] > 0), c.id
            assert ("wgrad.both" in lab) == (c["chunk"] > 0 and c["flush"] > 0), c.id
            if c["chunk"]:
                assert p["chunk"] <= c["chunk"] and p["nsplit"] > wgrad_plan(c["batch"], c["rows"], c["C"], c["K"])["nsplit"], c.id
            if "wgrad.nsplit_lt4" in lab:
                assert 1 <= p["nsplit"] <= 3, c.id
    assert {wgrad_plan(c["batch"], c["rows"], c["C"], c["K"], c["chunk"])["nsplit"] for c in CASES if "wgrad.nsplit_lt4" in c.labels} == {1, 2, 3}
    assert {c["rows"] for c in CASES if "wgrad.flushed" in c.labels} >= {27, 128, 129, 300}
    assert {(c["rows"], c["chunk"]) for c in CASES if "wgrad.chunked" in c.labels} == {(300, 32), (300, 64)}
    assert {c["K"] for c in CASES if c.kind == "gemm"} == {64, 132, 260} and {c["rows"] for c in CASES if c.kind == "gemm"} == {27, 130}


# ====================================================================================================================== inputs and references (GPU-free)
def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def inputs(c):
    g = c.gen()
    if c.kind == "filt":
        k, ch = c["K"], c["C"]
        return {"w": _rn(g, k, 3, 3, ch), "du22": _rn(g, 16, k, ch), "du44": _rn(g, 36, k, ch), "prior": _rn(g, k, 3, 3, ch)}
    if c.kind == "in":
        ch = c["C"]
        return {"x": _rn(g, c["N"], c["H"], c["W"], ch), "scale": torch.rand(ch, generator=g) + 0.5, "shift": _rn(g, ch, scale=0.3)}
    if c.kind == "dy":
        k = c["K"]
        coef = torch.stack([torch.rand(k, generator=g) + 0.5, _rn(g, k, scale=0.2), _rn(g, k, scale=0.3), _rn(g, k, scale=0.1)])
        return {"dy": _rn(g, c["N"], c["H"], c["W"], k), "x": _rn(g, c["N"], c["H"], c["W"], k), "coef": coef}
    if c.kind == "out":
        fam, k = c["fam"], c["K"]
        shape = (c["N"], c["H"], c["W"], k)
        inp = {"M": _rn(g, wo.POS[fam] ** 2, wo.tiles(fam, *shape[:3]), k)}
        if c["mode"] == "gate":
            inp.update({"gx": _rn(g, *shape), "scale": torch.rand(k, generator=g) + 0.5, "shift": _rn(g, k, scale=0.3), "mean": _rn(g, k, scale=0.2),
                        "invstd": torch.rand(k, generator=g) + 0.5})
            inp["bit"] = wo.gate_bit(inp["gx"], inp["scale"], inp["shift"])
            inp["mask"] = wo.pack_mask(inp["bit"])
        return inp
    b, rows, ch, k = c["batch"], c["rows"], c["C"], c["K"]
    if c.kind == "gemm":
        inp = {"a": _rn(g, b, rows, ch), "w": _rn(g, b, k, ch, scale=ch ** -0.5)}
        if c["addend"]:
            inp["addend"] = _rn(g, b, rows, k)
        if c["bias"]:
            inp["bias"] = _rn(g, k)
        return inp
    return {"x": _rn(g, b, rows, ch), "dy": _rn(g, b, rows, k)}


def refs(c, inp, dt):
    """name -> (tensor in dt, family | 'exact' | 'gemm'); for 'gemm' a third entry: the same product of the absolute values"""
    if c.kind == "filt":
        out = {}
        for fam, du in ((F22, "du22"), (F44, "du44")):
            fk = "exact" if fam == F22 else "f44"
            out[f"U{fam}"] = (wo.filter_transform(fam, inp["w"], dt), fk)
            out[f"dg{fam}"] = (wo.filter_grad(fam, inp[du], dt), fk)
            out[f"dg{fam}_acc"] = (wo.filter_grad(fam, inp[du], dt, prior=inp["prior"]), fk)
        return out
    if c.kind == "in":
        x, sc, sh = inp["x"], inp["scale"], inp["shift"]
        return {"V44": (wo.input_transform(F44, x, dt), "f44"), "V44xf": (wo.input_transform(F44, x, dt, sc, sh), "f44"),
                "V22": (wo.input_transform(F22, x, dt), "exact"), "V22xf": (wo.input_transform(F22, x, dt, sc, sh), "f22")}
    if c.kind == "dy":
        formed = wo.dyin(inp["dy"], inp["x"], inp["coef"], dt)
        return {"dM22": (wo.dy_transform(F22, inp["dy"], dt), "exact"), "dM44": (wo.dy_transform(F44, inp["dy"], dt), "f44"),
                "Vd44": (wo.input_transform(F44, inp["dy"], dt), "f44"),
                "dM44_dyin": (wo.dy_transform(F44, formed, dt), "f44"), "Vd44_dyin": (wo.input_transform(F44, formed, dt), "f44")}
    if c.kind == "out":
        fam = c["fam"]
        y = wo.output_transform(fam, inp["M"], c["N"], c["H"], c["W"], dt)
        fk = "exact" if fam == F22 else "f44"
        if c["mode"] == "gate":
            gy, sg, sgx = wo.gated(fam, y, inp["bit"], inp["gx"], inp["mean"], inp["invstd"], dt)
            return {"y": (gy, fk), "psum_g": (sg, FAMKEY[fam]), "psum_gx": (sgx, FAMKEY[fam])}
        out = {"y": (y, fk)}
        if c["mode"] == "stats":
            pm, pm2 = wo.stats_partials(fam, y, dt)
            out.update({"pmean": (pm, FAMKEY[fam]), "pm2": (pm2, FAMKEY[fam])})
        return out
    if c.kind == "gemm":
        def prod(a, w, absolute):
            y = torch.einsum("brc,bkc->brk", a, w)
            if "addend" in inp:
                y = y + (inp["addend"].abs() if absolute else inp["addend"]).to(dt)
            if "bias" in inp:
                y = y + (inp["bias"].abs() if absolute else inp["bias"]).to(dt)
            return y
        return {"y": (prod(inp["a"].to(dt), inp["w"].to(dt), False), "gemm", prod(inp["a"].to(dt).abs(), inp["w"].to(dt).abs(), True))}
    x, dy = inp["x"].to(dt), inp["dy"].to(dt)
    return {"dw": (torch.einsum("brk,brc->bkc", dy, x), "gemm", torch.einsum("brk,brc->bkc", dy.abs(), x.abs()))}


_REFS = {}


def case_refs(c):
    """(inputs, ref64, ref32) of a case, computed once and shared"""
    if c.id not in _REFS:
        inp = inputs(c)
        _REFS[c.id] = (inp, refs(c, inp, torch.float64), refs(c, inp, torch.float32))
    return _REFS[c.id]


def _e(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


def _m(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_is_well_conditioned(case):
    """(b), GPU-free"""
    inp, r64, r32 = case_refs(case)
    assert r64
    for name, ent in r64.items():
        ref, got32 = ent[0], r32[name][0]
        assert ref.dtype == torch.float64 and got32.dtype == torch.float32 and ref.shape == got32.shape
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0, f"{case.id} {name}"
        assert _e(got32, ref) <= COND and _m(got32, ref) <= COND, f"{case.id} {name}: ref32 is {_e(got32, ref):.2e} / {_m(got32, ref):.2e} from ref64"
    if case.kind == "out" and case["mode"] == "gate":
        frac = float(inp["bit"].float().mean())
        assert 0.2 < frac < 0.8, f"{case.id}: the gate passes {frac:.2f} of the elements"
        # rule (b'): the float64 sign IS the sign of the kernel's fmaf - an exact product and one rounding cannot cross zero
        a = inp["gx"].double() * inp["scale"].double() + inp["shift"].double()
        assert torch.equal(a > 0, inp["bit"]) and not bool((a == 0).any())


# ====================================================================================================================== GPU helpers
def _L():
    from ssv_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    L = _L()
    L.load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_WINO_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"source_sha16": L.source_sha16(), "device": torch.cuda.get_device_name(0), "floor": FLOOR, "factor": FACTOR,
                       "worst_ratio": WORST, "cases": REPORT}, f, indent=1, sort_keys=True)


class Run:
    """the buffers and results of one case"""

    def __init__(self, case, dev):
        self.case, self.dev, self.L = case, dev, _L()
        self.inputs, self.bufs, self.got, self.same = [], [], {}, []

    def up(self, t):
        """an input on the device, remembered for the bit-identical-afterwards check"""
        d = t.to(self.dev)
        self.inputs.append((d, t.clone()))
        return d

    def out(self, name, shape, guard=GUARD, prior=None, owned=True):
        """a 16-byte aligned view into a NaN-prefilled buffer with `guard` floats behind it; owned: every element must be written (a workspace: the guard only)"""
        n = math.prod(shape)
        buf = torch.full((n + guard,), float("nan"), device=self.dev)
        if prior is not None:
            buf[:n].copy_(prior.reshape(-1))
        assert buf.data_ptr() % 16 == 0
        self.bufs.append((name, buf, n, owned))
        return buf[:n].view(shape)

    def call(self, name, *args):
        assert name in self.case.entries or name in ("ssv_bn_apply", "ssv_split_planes"), f"{self.case.id} calls {name}, which its table row does not name"
        self.L.call(name, *args)

    def finish(self):
        """(d): outputs fully written, guards untouched, inputs unchanged"""
        torch.cuda.synchronize()
        for name, buf, n, owned in self.bufs:
            nan = torch.isnan(buf)
            assert not owned or not nan[:n].any(), f"{self.case.id} {name}: {int(nan[:n].sum())} of {n} elements never written (first at {int(nan[:n].nonzero()[0])})"
            assert nan[n:].all(), f"{self.case.id} {name}: wrote past the end of its buffer"
        for d, host in self.inputs:
            assert torch.equal(d.cpu(), host), f"{self.case.id}: an input changed"
        for name, a, b in self.same:
            assert torch.equal(a, b), f"{self.case.id} (e) {name}: {int((a != b).sum())} of {a.numel()} elements differ, max |a - b| {float((a - b).abs().max()):.3e}"


def _ratio(got, r32):
    return 0.0 if got <= FLOOR else (float("inf") if r32 == 0 else (got - FLOOR) / r32)


def check_bar(case, name, got, ref64, ref32, fam):
    """(a): e and m of got against those of ref32, or bitwise equality for the exact stages"""
    got = got.detach().cpu()
    assert got.shape == ref64.shape and torch.isfinite(got).all(), f"{case.id} {name}"
    rec = {"family": fam, "e_got": _e(got, ref64), "e_ref32": _e(ref32, ref64), "m_got": _m(got, ref64), "m_ref32": _m(ref32, ref64)}
    REPORT.setdefault(case.id, {})[name] = rec
    if fam == "exact":
        rec["bitwise"] = bool(torch.equal(got, ref32))
        print(f"{case.id} {name}: exact {rec['bitwise']}")
        assert rec["bitwise"], f"{case.id} {name}: {int((got != ref32).sum())} of {got.numel()} elements differ from ref32 in the kernel's order (max {float((got - ref32).abs().max()):.3e})"
        return
    rec["ratio_e"], rec["ratio_m"] = _ratio(rec["e_got"], rec["e_ref32"]), _ratio(rec["m_got"], rec["m_ref32"])
    WORST[fam] = max(WORST.get(fam, 0.0), rec["ratio_e"], rec["ratio_m"])
    print(f"{case.id} {name}: e {rec['e_got']:.3e} (ref32 {rec['e_ref32']:.3e}, x{rec['ratio_e']:.2f})  m {rec['m_got']:.3e} (ref32 {rec['m_ref32']:.3e}, x{rec['ratio_m']:.2f})")
    assert rec["e_got"] <= FACTOR[fam] * rec["e_ref32"] + FLOOR, f"{case.id} {name}: e {rec['e_got']:.3e} > {FACTOR[fam]} x {rec['e_ref32']:.3e} + {FLOOR:.1e}"
    assert rec["m_got"] <= FACTOR[fam] * rec["m_ref32"] + FLOOR, f"{case.id} {name}: m {rec['m_got']:.3e} > {FACTOR[fam]} x {rec['m_ref32']:.3e} + {FLOOR:.1e}"


def check_rows(case, name, got, ref64, ref32, fam):
    """(c): a partial buffer row by row (group by group) under (a)'s bar; the worst row is reported"""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, f"{case.id} {name}: {tuple(got.shape)} partial rows for {tuple(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{case.id} {name}: non-finite partials"
    worst = (0.0, 0.0, -1)
    bad = []
    for g in range(got.shape[0]):
        eg, e32, mg, m32 = _e(got[g], ref64[g]), _e(ref32[g], ref64[g]), _m(got[g], ref64[g]), _m(ref32[g], ref64[g])
        r = max(_ratio(eg, e32), _ratio(mg, m32))
        if r > worst[0]:
            worst = (r, eg, g)
        if eg > FACTOR[fam] * e32 + FLOOR or mg > FACTOR[fam] * m32 + FLOOR:
            bad.append((g, eg, e32, mg, m32))
    REPORT.setdefault(case.id, {})[name] = {"family": fam, "groups": int(got.shape[0]), "worst_row_ratio": worst[0], "worst_row_e": worst[1], "worst_row": worst[2]}
    WORST[fam] = max(WORST.get(fam, 0.0), worst[0])
    print(f"{case.id} {name}: {got.shape[0]} groups, worst row {worst[2]} x{worst[0]:.2f} (e {worst[1]:.3e})")
    assert not bad, f"{case.id} {name}: {len(bad)} of {got.shape[0]} groups over the bar; first (group, e, e32, m, m32): {bad[0]}"


# ====================================================================================================================== the runners
# The four transform kinds run in two parts: _call_<kind> makes every library call of the case on guarded buffers, verifies (d) and the identities (e) and
# returns the arrays by name (with the library's host answers); _check_<kind> holds them to (a) and (c).  tools/same_bits.py dumps what the first part returns.
def _call_filt(c, r):
    inp, _, _ = case_refs(c)
    L, k, ch = r.L, c["K"], c["C"]
    w, prior = r.up(inp["w"]), inp["prior"]
    o = {}
    for fam, dun in ((F22, "du22"), (F44, "du44")):
        p = wo.POS[fam] ** 2
        du = r.up(inp[dun])
        u, u2 = r.out(f"U{fam}", (p, k, ch)), r.out(f"U{fam}'", (p, k, ch))
        for t in (u, u2):
            r.call(PFX[fam] + "filter_transform", k, ch, L.ptr(w), L.ptr(t), L.stream())
        dg, dg2 = r.out(f"dg{fam}", (k, 3, 3, ch)), r.out(f"dg{fam}'", (k, 3, 3, ch))
        for t in (dg, dg2):
            r.call(PFX[fam] + "filter_grad", k, ch, L.ptr(du), L.ptr(t), 0, L.stream())
        dg0 = r.out(f"dg{fam}_zero", (k, 3, 3, ch), prior=torch.zeros(k, 3, 3, ch))
        dga = r.out(f"dg{fam}_acc", (k, 3, 3, ch), prior=prior)
        for t in (dg0, dga):
            r.call(PFX[fam] + "filter_grad", k, ch, L.ptr(du), L.ptr(t), 1, L.stream())
        r.same += [(f"second filter_transform {fam}", u, u2), (f"second filter_grad {fam}", dg, dg2), (f"accumulate on zero == overwrite {fam}", dg0, dg)]
        o.update({f"U{fam}": u, f"dg{fam}": dg, f"dg{fam}_acc": dga})
    r.finish()
    return o


def _check_filt(c, o):
    inp, r64, r32 = case_refs(c)
    for fam in (F22, F44):
        for name in (f"U{fam}", f"dg{fam}", f"dg{fam}_acc"):
            check_bar(c, name, o[name], r64[name][0], r32[name][0], r64[name][1])
        # a seeded prior: prior + overwrite within one rounding
        want = inp["prior"].double() + o[f"dg{fam}"].cpu().double()
        err = (o[f"dg{fam}_acc"].cpu().double() - want).abs()
        assert bool((err <= U * want.abs() + 1e-45).all()), f"{c.id} dg{fam}_acc: {float((err / want.abs().clamp_min(1e-30)).max()) / U:.2f} roundings from prior + overwrite"


def _bn_apply_relu(r, x, sc, sh):
    L = r.L
    a = torch.empty_like(x)
    r.call("ssv_bn_apply", x.numel() // x.shape[-1], x.shape[-1], L.ptr(x), L.ptr(sc), L.ptr(sh), None, None, None, 1, L.ptr(a), None, L.stream())
    return a


def _call_in(c, r):
    inp, _, _ = case_refs(c)
    L, n, h, w, ch = r.L, c["N"], c["H"], c["W"], c["C"]
    lib = L.load()
    t4, t2 = int(lib.ssv_wino44_tiles(n, h, w)), int(lib.ssv_wino_tiles(n, h, w))
    assert (t4, t2) == (wo.tiles(F44, n, h, w), wo.tiles(F22, n, h, w))
    x, sc, sh = r.up(inp["x"]), r.up(inp["scale"]), r.up(inp["shift"])
    act = _bn_apply_relu(r, x, sc, sh)

    def f44(name, src, aff, both):
        v = r.out(name, (36, t4, ch))
        v2 = r.out(name + ".V2", (16, t2, ch)) if both else None
        r.call("ssv_wino44_input_transform", n, h, w, ch, L.ptr(src), L.ptr(sc) if aff else None, L.ptr(sh) if aff else None, L.ptr(v), L.ptr(v2), L.stream())
        return v, v2

    def f22(name, src, aff):
        v = r.out(name, (16, t2, ch))
        r.call("ssv_wino_input_transform", n, h, w, ch, L.ptr(src), L.ptr(sc) if aff else None, L.ptr(sh) if aff else None, L.ptr(v), L.stream())
        return v

    v_a, _ = f44("V44", x, False, False)
    v_b, v2_b = f44("V44+V2", x, False, True)
    vx_a, _ = f44("V44xf", x, True, False)
    vx_b, v2x_b = f44("V44xf+V2", x, True, True)
    vm, _ = f44("V44(act)", act, False, False)
    w_p, w_x, w_m, w_p2 = f22("V22", x, False), f22("V22xf", x, True), f22("V22(act)", act, False), f22("V22'", x, False)
    v_a2, _ = f44("V44'", x, False, False)
    r.same += [("V with and without V2", v_a, v_b), ("V2 == ssv_wino_input_transform", v2_b, w_p), ("fused V with and without V2", vx_a, vx_b),
               ("fused V2 == fused ssv_wino_input_transform", v2x_b, w_x), ("fused F(4x4) input == transform of ssv_bn_apply's activation", vx_a, vm),
               ("fused F(2x2) input == transform of ssv_bn_apply's activation", w_x, w_m), ("second F(2x2) call", w_p, w_p2), ("second F(4x4) call", v_a, v_a2)]
    r.finish()
    return {"V44": v_a, "V44xf": vx_a, "V22": w_p, "V22xf": w_x, "V44+V2": v_b, "V44+V2.V2": v2_b, "V44xf+V2": vx_b, "V44xf+V2.V2": v2x_b, "tiles44": t4, "tiles22": t2}


def _check_in(c, o):
    _, r64, r32 = case_refs(c)
    for name in ("V44", "V44xf", "V22", "V22xf"):
        check_bar(c, name, o[name], r64[name][0], r32[name][0], r64[name][1])


def _call_dy(c, r):
    inp, _, _ = case_refs(c)
    L, n, h, w, k = r.L, c["N"], c["H"], c["W"], c["K"]
    lib = L.load()
    t4, t2 = int(lib.ssv_wino44_tiles(n, h, w)), int(lib.ssv_wino_tiles(n, h, w))
    dy, x, coef = r.up(inp["dy"]), r.up(inp["x"]), r.up(inp["coef"])
    dm22, dm22b = r.out("dM22", (16, t2, k)), r.out("dM22'", (16, t2, k))
    for t in (dm22, dm22b):
        r.call("ssv_wino_dy_transform", n, h, w, k, L.ptr(dy), L.ptr(t), L.stream())
    dm44 = r.out("dM44", (36, t4, k))
    r.call("ssv_wino44_dy_transform", n, h, w, k, L.ptr(dy), L.ptr(dm44), L.stream())
    vin = torch.empty((36, t4, k), device=r.dev)
    L.call("ssv_wino44_input_transform", n, h, w, k, L.ptr(dy), None, None, L.ptr(vin), None, L.stream())          # the identity's other side (its own case: kind `in`)
    vd, dmb = r.out("Vd44", (36, t4, k)), r.out("dM44(both)", (36, t4, k))
    vd2, dmb2 = r.out("Vd44'", (36, t4, k)), r.out("dM44(both)'", (36, t4, k))
    for a, b in ((vd, dmb), (vd2, dmb2)):
        r.call("ssv_wino44_dy_transform_both", n, h, w, k, L.ptr(dy), None, L.ptr(a), L.ptr(b), L.stream())
    st = L.BnDyin(L.ptr(x), L.ptr(coef))
    vdf, dmf = r.out("Vd44_dyin", (36, t4, k)), r.out("dM44_dyin", (36, t4, k))
    r.call("ssv_wino44_dy_transform_both", n, h, w, k, L.ptr(dy), C.byref(st), L.ptr(vdf), L.ptr(dmf), L.stream())
    r.same += [("both: Vd == ssv_wino44_input_transform(dy)", vd, vin), ("both: dM == ssv_wino44_dy_transform(dy)", dmb, dm44), ("second dy_transform", dm22, dm22b),
               ("second dy_transform_both (Vd)", vd, vd2), ("second dy_transform_both (dM)", dmb, dmb2)]
    r.finish()
    return {"dM22": dm22, "dM44": dm44, "Vd44": vd, "dM44(both)": dmb, "dM44_dyin": dmf, "Vd44_dyin": vdf, "tiles44": t4, "tiles22": t2}


def _check_dy(c, o):
    _, r64, r32 = case_refs(c)
    for name in ("dM22", "dM44", "Vd44", "dM44_dyin", "Vd44_dyin"):
        check_bar(c, name, o[name], r64[name][0], r32[name][0], r64[name][1])


def _gate_struct(r, inp, k, groups, mask):
    L = r.L
    keep = {n_: r.up(inp[n_]) for n_ in (("gx", "mean", "invstd", "mask") if mask else ("gx", "mean", "invstd", "scale", "shift"))}
    tag = "mask" if mask else "affine"
    pg, pgx = r.out(f"psum_g({tag})", (groups, k)), r.out(f"psum_gx({tag})", (groups, k))
    st = L.BnGate(L.ptr(keep["gx"]), L.ptr(keep.get("scale")), L.ptr(keep.get("shift")), L.ptr(keep.get("mask")), L.ptr(keep["mean"]), L.ptr(keep["invstd"]),
                  L.ptr(pg), L.ptr(pgx), None, None, None, None)
    return st, pg, pgx, keep


def _call_out(c, r):
    inp, _, _ = case_refs(c)
    L, fam, mode, n, h, w, k = r.L, c["fam"], c["mode"], c["N"], c["H"], c["W"], c["K"]
    lib = L.load()
    entry = PFX[fam] + "output_transform"
    groups = int(lib.ssv_wino_groups(n, h, w)) if fam == F22 else int(lib.ssv_wino44_groups(n, h, w, 1 if mode == "stats" else 0))
    assert groups == wo.groups(fam, n, h, w, mode == "stats")
    m = r.up(inp["M"])
    o = {"groups": groups}
    if mode == "plain":
        y, y2 = r.out("y", (n, h, w, k)), r.out("y'", (n, h, w, k))
        for t in (y, y2):
            r.call(entry, n, h, w, k, L.ptr(m), L.ptr(t), None, None, None, L.stream())
        r.same.append(("second call", y, y2))
    elif mode == "stats":
        rpg = int(lib.ssv_wino_stats_rows_per_group(n, h, w)) if fam == F22 else int(lib.ssv_wino44_stats_rows_per_group(n, h, w))
        assert rpg == wo.stats_rows_per_group(fam, n, h, w) > 0
        y, pm, pm2 = r.out("y", (n, h, w, k)), r.out("pmean", (groups, k)), r.out("pm2", (groups, k))
        y2, pmb, pm2b = r.out("y'", (n, h, w, k)), r.out("pmean'", (groups, k)), r.out("pm2'", (groups, k))
        yp = r.out("y(plain)", (n, h, w, k))
        r.call(entry, n, h, w, k, L.ptr(m), L.ptr(y), L.ptr(pm), L.ptr(pm2), None, L.stream())
        r.call(entry, n, h, w, k, L.ptr(m), L.ptr(y2), L.ptr(pmb), L.ptr(pm2b), None, L.stream())
        r.call(entry, n, h, w, k, L.ptr(m), L.ptr(yp), None, None, None, L.stream())
        r.same += [("second call (y)", y, y2), ("second call (pmean)", pm, pmb), ("second call (pm2)", pm2, pm2b), ("y with and without the statistics", y, yp)]
        o.update({"pmean": pm, "pm2": pm2, "rows_per_group": rpg})
    else:
        sta, pga, pgxa, keep_a = _gate_struct(r, inp, k, groups, mask=False)
        stm, pgm, pgxm, keep_m = _gate_struct(r, inp, k, groups, mask=True)
        stb, pgb, pgxb, keep_b = _gate_struct(r, inp, k, groups, mask=False)
        y, ym, y2 = r.out("y(affine)", (n, h, w, k)), r.out("y(mask)", (n, h, w, k)), r.out("y(affine)'", (n, h, w, k))
        for st, t in ((sta, y), (stm, ym), (stb, y2)):
            r.call(entry, n, h, w, k, L.ptr(m), L.ptr(t), None, None, C.byref(st), L.stream())
        r.same += [("mask gate == affine gate (y)", ym, y), ("mask gate == affine gate (psum_g)", pgm, pga), ("mask gate == affine gate (psum_gx)", pgxm, pgxa),
                   ("second call (y)", y, y2), ("second call (psum_g)", pga, pgb), ("second call (psum_gx)", pgxa, pgxb)]
        o.update({"psum_g": pga, "psum_gx": pgxa, "y(mask)": ym, "psum_g(mask)": pgm, "psum_gx(mask)": pgxm})
    r.finish()
    o["y"] = y
    return o


def _check_out(c, o):
    inp, r64, r32 = case_refs(c)
    fam, mode, n, h, w = c["fam"], c["mode"], c["N"], c["H"], c["W"]
    fk = FAMKEY[fam]
    y = o["y"]
    if mode == "stats":
        ycpu = y.cpu()
        (m64, v64), (m32, v32) = wo.stats_partials(fam, ycpu, torch.float64), wo.stats_partials(fam, ycpu, torch.float32)
        assert [int(x.numel()) for x in wo.group_rows(fam, n, h, w, True)][:-1] == [o["rows_per_group"]] * (o["groups"] - 1)
        check_rows(c, "pmean", o["pmean"], m64, m32, fk)
        check_rows(c, "pm2", o["pm2"], v64, v32, fk)
    elif mode == "gate":
        ones = torch.ones(y.shape, dtype=torch.bool)
        ycpu = y.cpu()
        assert torch.equal(ycpu != 0, inp["bit"] & (ycpu != 0)), f"{c.id}: a gated-off element is not zero"
        _, g64, gx64 = wo.gated(fam, ycpu, ones, inp["gx"], inp["mean"], inp["invstd"], torch.float64)
        _, g32, gx32 = wo.gated(fam, ycpu, ones, inp["gx"], inp["mean"], inp["invstd"], torch.float32)
        check_rows(c, "psum_g", o["psum_g"], g64, g32, fk)
        check_rows(c, "psum_gx", o["psum_gx"], gx64, gx32, fk)
    check_bar(c, "y", y, r64["y"][0], r32["y"][0], r64["y"][1])


CALLERS = {"filt": (_call_filt, _check_filt), "in": (_call_in, _check_in), "dy": (_call_dy, _check_dy), "out": (_call_out, _check_out)}


def _run_transform(c, r):
    call, check = CALLERS[c.kind]
    check(c, call(c, r))


def _gemm_check(c, name, got, ref64, amag, arith):
    """(a) for the products: tests/test_gpu_conv_forms.py's element-wise bound"""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{c.id} {name} [{arith}]: non-finite values"
    err = (got.double() - ref64).abs()
    bound = GEMM_TAU * U * amag + 1e-30 + 1e-3 * U * float(amag.max())
    ratio, rel = float((err / bound).max()), _e(got, ref64)
    REPORT.setdefault(c.id, {})[f"{name}[{arith}]"] = {"family": "gemm", "err_over_bound": ratio, "e_got": rel}
    WORST["gemm"] = max(WORST.get("gemm", 0.0), ratio)
    print(f"{c.id} {name} [{arith}]: |err| / bound {ratio:.3f}, e {rel:.3e}")
    assert ratio <= 1.0, f"{c.id} {name} [{arith}]: {int((err > bound).sum())} of {err.numel()} elements over the bound (worst |err| / bound {ratio:.2f})"
    return rel


def _run_gemm(c, r):
    inp, r64, _ = case_refs(c)
    L, b, rows, ch, k = r.L, c["batch"], c["rows"], c["C"], c["K"]
    a, w = r.up(inp["a"]), r.up(inp["w"])
    add = inp.get("addend")
    bias = r.up(inp["bias"]) if c["bias"] else None
    ref, amag = r64["y"][0], r64["y"][2]
    planes = torch.zeros((3, b * k * ch), dtype=torch.int16, device=r.dev)
    r.call("ssv_split_planes", b * k * ch, L.ptr(w), L.ptr(planes), L.stream())
    # fp32 MFMA has no epilogue operands: its reference is the bare product
    bare64 = torch.einsum("brc,bkc->brk", inp["a"].double(), inp["w"].double())
    bare_mag = torch.einsum("brc,bkc->brk", inp["a"].double().abs(), inp["w"].double().abs())
    y, y2 = r.out("y[f32]", (b, rows, k)), r.out("y[f32]'", (b, rows, k))
    for o in (y, y2):
        r.call("ssv_gemm_batched", b, rows, ch, k, L.ptr(a), L.ptr(w), L.ptr(o), L.stream())
    ys, ys2 = r.out("y[bf16x3]", (b, rows, k), prior=add), r.out("y[bf16x3]'", (b, rows, k), prior=add)
    for o in (ys, ys2):                                                  # the addend in place: it is read from the output's own memory
        r.call("ssv_gemm_batched_split", b, rows, ch, k, L.ptr(a), L.ptr(planes), L.ptr(o), L.ptr(bias), L.ptr(o) if add is not None else None, L.stream())
    r.same += [("second ssv_gemm_batched", y, y2), ("second ssv_gemm_batched_split", ys, ys2)]
    if add is not None or bias is not None:
        yb = r.out("y[bf16x3, bare]", (b, rows, k))
        r.call("ssv_gemm_batched_split", b, rows, ch, k, L.ptr(a), L.ptr(planes), L.ptr(yb), None, None, L.stream())
    else:
        yb = ys
    r.finish()
    e32 = _gemm_check(c, "y", y, bare64, bare_mag, "f32")
    _gemm_check(c, "y", ys, ref, amag, "bf16x3")
    e16 = _gemm_check(c, "y(bare)", yb, bare64, bare_mag, "bf16x3")
    REPORT[c.id]["bf16x3_over_f32"] = e16 / e32
    assert e16 <= GEMM_BF16_BAR * e32 + 1e-9, f"{c.id}: bf16x3 is {e16:.3e} from fp64, fp32 MFMA {e32:.3e} (x{e16 / e32:.3f})"


def _run_wgrad(c, r):
    inp, r64, _ = case_refs(c)
    L, b, rows, ch, k, chunk, flush = r.L, c["batch"], c["rows"], c["C"], c["K"], c["chunk"], c["flush"]
    lib = L.load()
    x, dy = r.up(inp["x"]), r.up(inp["dy"])
    ref, amag = r64["dw"][0], r64["dw"][2]
    blocked = bool(chunk or flush)
    need = int(lib.ssv_gemm_batched_wgrad_blocked_workspace_bytes(b, rows, ch, k, chunk)) if blocked else int(lib.ssv_gemm_batched_wgrad_workspace_bytes(b, rows, ch, k))
    plan = wgrad_plan(b, rows, ch, k, chunk)
    assert need == b * plan["nsplit"] * k * ch * 4, f"{c.id}: the library plans {need} workspace bytes, the restated plan {plan}"
    assert int(lib.ssv_gemm_batched_wgrad_blocked_workspace_bytes(b, rows, ch, k, chunk)) == need

    def one(tag, split):
        ws = r.out(f"ws[{tag}]", (need // 4,), guard=WS_GUARD, owned=False)
        dw = r.out(f"dw[{tag}]", (b, k, ch))
        if split:
            r.call("ssv_gemm_batched_wgrad_split", b, rows, ch, k, L.ptr(x), L.ptr(dy), L.ptr(dw), chunk, flush, L.ptr(ws), need, L.stream())
        elif blocked:
            r.call("ssv_gemm_batched_wgrad_blocked", b, rows, ch, k, L.ptr(x), L.ptr(dy), L.ptr(dw), chunk, flush, L.ptr(ws), need, L.stream())
        else:
            r.call("ssv_gemm_batched_wgrad", b, rows, ch, k, L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(ws), need, L.stream())
        return dw

    d32, d32b, d16, d16b = one("f32", False), one("f32'", False), one("bf16x3", True), one("bf16x3'", True)
    r.same += [("second fp32 call", d32, d32b), ("second bf16x3 call", d16, d16b)]
    r.finish()
    e32 = _gemm_check(c, "dw", d32, ref, amag, "f32")
    e16 = _gemm_check(c, "dw", d16, ref, amag, "bf16x3")
    REPORT[c.id]["bf16x3_over_f32"] = e16 / e32
    assert e16 <= GEMM_BF16_BAR * e32 + 1e-9, f"{c.id}: bf16x3 is {e16:.3e} from fp64, fp32 MFMA {e32:.3e} (x{e16 / e32:.3f})"


RUNNERS = {"filt": _run_transform, "in": _run_transform, "dy": _run_transform, "out": _run_transform, "gemm": _run_gemm, "wgrad": _run_wgrad}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_stage_against_fp64(dev, case):
    RUNNERS[case.kind](case, Run(case, dev))


# ====================================================================================================================== (f) refusals
def _refusals():
    """(id, entry point, what is wrong): built lazily on the device by _refusal_args"""
    return ["out22-K24", "out44-K24", "out22-stats-9x5", "out22-pmean-without-pm2", "out44-pmean-without-pm2", "out22-stats-and-gate", "out44-stats-and-gate", "out22-gate-x2",
            "out44-gate-x2", "out22-gate-mask-and-scale", "out44-gate-mask-and-scale", "out22-pointer-off-by-4", "out44-pointer-off-by-4", "in22-pointer-off-by-4",
            "in44-pointer-off-by-4", "dy44-both-pointer-off-by-4", "gemm-C48", "gemm-split-bias-batch2", "wgrad-blocked-chunk16", "wgrad-blocked-flush64", "wgrad-blocked-0-0",
            "wgrad-split-chunk16", "wgrad-ws-one-byte-short", "wgrad-blocked-ws-one-byte-short", "wgrad-split-ws-one-byte-short"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", _refusals())
def test_refusals_leave_outputs_untouched(dev, what):
    L = _L()
    lib = L.load()
    nan = lambda *s: torch.full(s, float("nan"), device=dev)                                                # noqa: E731
    rn = lambda *s: torch.randn(*s, device=dev)                                                              # noqa: E731
    p = L.ptr
    outs = []
    kind = what.split("-")[0]
    if kind in ("out22", "out44"):
        fam = F22 if kind == "out22" else F44
        n, h, w, k = (2, 9, 5, 32) if "9x5" in what else (2, 8, 8, 24 if "K24" in what else 32)
        t = wo.tiles(fam, n, h, w)
        m, y, pm, pm2, pg, pgx = rn(wo.POS[fam] ** 2, t, k), nan(n, h, w, k), nan(8, k), nan(8, k), nan(8, k), nan(8, k)
        gx, sc, sh, mean, inv, mask = rn(n, h, w, k), rn(k), rn(k), rn(k), rn(k), torch.zeros(n * h * w * k // 4, dtype=torch.uint8, device=dev)
        outs = [y, pm, pm2, pg, pgx]

        def gate(scale=None, shift=None, mask=None, x2=None):
            second = (None, None, None) if x2 is None else (mean, inv, pm)
            return L.BnGate(p(gx), p(scale), p(shift), p(mask), p(mean), p(inv), p(pg), p(pgx), p(x2), p(second[0]), p(second[1]), p(second[2]))

        args = {"K24": (p(m), p(y), None, None, None), "stats": (p(m), p(y), p(pm), p(pm2), None), "pmean": (p(m), p(y), p(pm), None, None),
                "pointer": (p(m) + 4, p(y), None, None, None)}
        key = what.split("-")[1]
        if key == "stats" and "gate" in what:
            a = (p(m), p(y), p(pm), p(pm2), C.byref(gate(scale=sc, shift=sh)))
        elif key == "gate":
            st = gate(mask=mask, x2=gx) if "x2" in what else gate(mask=mask, scale=sc, shift=sh)
            a = (p(m), p(y), None, None, C.byref(st))
        else:
            a = args[key]
        rc = getattr(lib, PFX[fam] + "output_transform")(n, h, w, k, *a, L.stream())
    elif kind in ("in22", "in44"):
        n, h, w, ch = 2, 8, 8, 8
        x, v = rn(n, h, w, ch), nan(36, wo.tiles(F22, n, h, w), ch)
        outs = [v]
        rc = lib.ssv_wino_input_transform(n, h, w, ch, p(x) + 4, None, None, p(v), L.stream()) if kind == "in22" else \
            lib.ssv_wino44_input_transform(n, h, w, ch, p(x), None, None, p(v) + 4, None, L.stream())
    elif kind == "dy44":
        n, h, w, k = 2, 8, 8, 8
        dy, vd, dm = rn(n, h, w, k), nan(36, 8, k), nan(36, 8, k)
        outs = [vd, dm]
        rc = lib.ssv_wino44_dy_transform_both(n, h, w, k, p(dy), None, p(vd), p(dm) + 4, L.stream())
    elif kind == "gemm":
        b, rows, ch, k = 2, 40, (48 if "C48" in what else 64), 64
        a, w_, y, bias = rn(b, rows, ch), rn(b, k, ch), nan(b, rows, k), rn(k)
        outs = [y]
        if "C48" in what:
            rc = lib.ssv_gemm_batched(b, rows, ch, k, p(a), p(w_), p(y), L.stream())
        else:
            pl = torch.zeros(3, b * k * ch, dtype=torch.int16, device=dev)
            L.call("ssv_split_planes", b * k * ch, p(w_), p(pl), L.stream())
            rc = lib.ssv_gemm_batched_split(b, rows, ch, k, p(a), p(pl), p(y), p(bias), None, L.stream())
    else:
        b, rows, ch, k = 16, 300, 36, 64
        x, dy, dw = rn(b, rows, ch), rn(b, rows, k), nan(b, k, ch)
        chunk, flush = {"chunk16": (16, 0), "flush64": (0, 64), "0": (0, 0)}.get(what.split("-")[2], (64 if "blocked" in what else 0, 0))
        need = int(lib.ssv_gemm_batched_wgrad_blocked_workspace_bytes(b, rows, ch, k, chunk if chunk >= 32 else 0))
        assert need > 0
        ws = nan(need // 4 + 4)
        outs = [dw, ws]
        nbytes = need - 1 if "short" in what else need
        if "blocked" in what:
            rc = lib.ssv_gemm_batched_wgrad_blocked(b, rows, ch, k, p(x), p(dy), p(dw), chunk, flush, p(ws), nbytes, L.stream())
        elif "split" in what:
            rc = lib.ssv_gemm_batched_wgrad_split(b, rows, ch, k, p(x), p(dy), p(dw), chunk, flush, p(ws), nbytes, L.stream())
        else:
            rc = lib.ssv_gemm_batched_wgrad(b, rows, ch, k, p(x), p(dy), p(dw), p(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{what}: accepted"
    msg = lib.ssv_last_error().decode()
    assert msg and ("ssv_wino" in msg or "ssv_gemm_batched" in msg), f"{what}: ssv_last_error is {msg!r}"
    for o in outs:
        assert torch.isnan(o).all(), f"{what}: a refused call wrote {int((~torch.isnan(o)).sum())} elements"


# ====================================================================================================================== cache coherence (through ops)
def _coherence_products(ops, dev):
    """name -> (run(w) -> result, fp64 reference(w64) -> tensor, counted library calls of one cold run)"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(77)
    n, h, w_, c, k = 2, 8, 8, 128, 128
    x, dy = torch.randn(n, h, w_, c, generator=g), torch.randn(n, h, w_, k, generator=g)
    xd, dyd = x.to(dev), dy.to(dev)
    nchw = lambda t: t.permute(0, 3, 1, 2)                                                                   # noqa: E731
    fwd64 = lambda w64: F.conv2d(nchw(x.double()), w64, padding=1).permute(0, 2, 3, 1)                       # noqa: E731
    dgr64 = lambda w64: F.conv_transpose2d(nchw(dy.double()), w64, padding=1).permute(0, 2, 3, 1)           # noqa: E731
    return {
        "_transposed_filter": (lambda w: ops.conv2d_dgrad(dyd, w, (n, h, w_, c), stride=1, pad=1), dgr64),
        "_wino_filter": (lambda w: _with(ops, False, lambda: ops.wino_conv2d_fwd(xd, w)[0]), fwd64),
        "_wino_filter(transposed)": (lambda w: _with(ops, False, lambda: ops.wino_conv2d_dgrad(dyd, w)), dgr64),
        "_wino44_filter": (lambda w: ops.wino44_conv2d_fwd(xd, w)[0], fwd64),
        "_wino44_filter(transposed)": (lambda w: ops.wino44_conv2d_dgrad(dyd, w), dgr64),
        "_planes": (lambda w: ops.conv2d_fwd(xd, w, stride=1, pad=1), fwd64),
    }


def _with(ops, wino44, fn):
    prev, ops.WINOGRAD44 = ops.WINOGRAD44, wino44
    try:
        return fn()
    finally:
        ops.WINOGRAD44 = prev


COHERENCE = ("_transposed_filter", "_wino_filter", "_wino_filter(transposed)", "_wino44_filter", "_wino44_filter(transposed)", "_planes")
# the product's own tolerance against fp64 (relative l2): tests/test_gpu_winograd.py / test_gpu_winograd44.py / test_gpu_split.py
COHERENCE_TOL = {"_transposed_filter": 2e-6, "_wino_filter": 2e-6, "_wino_filter(transposed)": 2e-6, "_wino44_filter": 4e-6, "_wino44_filter(transposed)": 4e-6, "_planes": 2e-6}


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ("f32", "bf16x3"))
@pytest.mark.parametrize("which", COHERENCE)
def test_cached_filters_follow_in_place_edits(dev, which, arith):
    """A torch-level in-place edit of a channels-last filter between two calls - WITHOUT ops.invalidate_weight_caches() - must reach every cached image of it: the
    transposed filter of the stride-1 data gradient, both Winograd-transformed filters in both orientations, and the bf16 planes.  And the reverse: an unedited
    weight hits the cache (one transform per weight and step, which graph.py's capture relies on), and invalidate_weight_caches() empties it."""
    from ssv_amd import _lib, ops
    run, ref64 = _coherence_products(ops, dev)[which]
    wt = torch.randn(128, 128, 3, 3, generator=torch.Generator().manual_seed(5)) * (2.0 / (9 * 128)) ** 0.5
    w = wt.to(dev).contiguous(memory_format=torch.channels_last)
    counted = ("ssv_wino_filter_transform", "ssv_wino44_filter_transform", "ssv_filter_transpose", "ssv_split_planes")
    calls = []
    real = _lib.call

    def counting(name, *args):
        if name in counted:
            calls.append(name)
        return real(name, *args)

    with ops.arithmetic(arith):
        _lib.call = ops.call = counting
        try:
            ops.invalidate_weight_caches()
            first = run(w).clone()
            cold = list(calls)
            again = run(w)
            assert calls == cold, f"{which}: an unedited weight missed the cache ({calls[len(cold):]})"
            assert torch.equal(again, first)
            w.mul_(-2.0)                                                 # a torch op: the version moves, no invalidate_weight_caches()
            second = run(w).clone()
            assert len(calls) == 2 * len(cold), f"{which}: the edited weight ran {calls[len(cold):]} (a cold run: {cold})"
            ops.invalidate_weight_caches()
            assert not ops._WT_CACHE and not ops._WINO_U and not ops._PLANES
            third = run(w)
            assert calls[2 * len(cold):] == cold and torch.equal(third, second), f"{which}: after invalidate_weight_caches() the cache refills with the same bits"
        finally:
            _lib.call = ops.call = real
            ops.invalidate_weight_caches()
    if which != "_planes" or arith == "bf16x3":
        assert cold, f"{which} [{arith}]: the product never built the cached image this case is about"
    r1, r2 = ref64(wt.double()), ref64(-2.0 * wt.double())
    e1, e2 = _e(first.cpu(), r1), _e(second.cpu(), r2)
    print(f"{which} [{arith}]: {cold}; e(first) {e1:.3e}, e(second against -2 x) {e2:.3e}")
    assert e1 <= COHERENCE_TOL[which], f"{which} [{arith}]: first result {e1:.3e} from fp64"
    assert e2 <= COHERENCE_TOL[which], f"{which} [{arith}]: after w.mul_(-2) the result is {e2:.3e} from the fp64 product of the EDITED filter (stale cache: about 1.5)"
    if arith == "f32":
        assert torch.equal(second, -2.0 * first), f"{which} [{arith}]: a filter scaled by a power of two scales an fp32 result exactly"
