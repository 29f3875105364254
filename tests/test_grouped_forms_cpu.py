"""GPU-free: the case table of tests/test_gpu_grouped_forms.py is honest.  Every documented (branch, form) has a case and every case a documented branch; the
form labels follow the dispatch; the restatement of tests/grouped_oracle.py shows per case what its label claims (spans that leave channel chunks out, a tile
holding two groups, skipped and worked tiles, a short last row chunk); the restated weight-gradient plan equals the library's own answer
(ssv_conv2d_wgrad_grouped_workspace_bytes is host code); the fp64 references are conditioned and equal the dense convolution on the expanded bank."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import grouped_oracle as go
import test_gpu_grouped_forms as gf
from ssv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_BRANCH = {}
for _c in gf.CASES:
    for _b in _c.branches:
        BY_BRANCH.setdefault(_b, []).append(_c)


def defines(src, name):
    """Does the C++ text hold a DEFINITION of function `name` (a declarator starting a line whose parameter list is followed by a body, not a `;`)?"""
    for m in re.finditer(r"^[A-Za-z_][^\n;{}()]*\b%s\(" % re.escape(name), src, re.M):
        depth, i = 1, m.end()
        while depth and i < len(src):
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        if re.match(r"\s*\{", src[i:]):
            return True
    return False


def test_case_table_covers_every_documented_branch():
    doc = gf.documented_branches()
    assert len({b for b, _ in doc}) == 29 and len(doc) > 50
    missing = doc - gf.covered_branches()
    assert not missing, f"documented branches without a case: {sorted(missing)}"
    stray = {b for c in gf.CASES for b in c.branches} - {b for b, _ in doc}
    assert not stray, f"cases name undocumented branches: {sorted(stray)}"
    undocumented_forms = gf.covered_branches() - doc
    assert not undocumented_forms, f"cases take forms their branch does not document: {sorted(undocumented_forms)}"
    ids = [c.id for c in gf.CASES]
    assert len(ids) == len(set(ids))
    assert all(cid in gf.BY_ID for cid, _ in gf.POISON)
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "conv_mfma.hip")).read()
    named = set(re.findall(r"conv_mfma\.hip:([A-Za-z_]\w*)", gf.__doc__))
    assert len(named) >= 8
    for name in sorted(named):
        assert defines(src, name), f"the docstring names conv_mfma.hip:{name}, which the source does not define"
    assert not defines(src, "no_such_function_anywhere")
    for name in ("ssv_conv2d_fwd_grouped", "ssv_conv2d_dgrad_grouped", "ssv_conv2d_wgrad_grouped", "ssv_conv2d_wgrad_grouped_workspace_bytes"):
        assert defines(src, name), name


def test_form_labels_follow_the_dispatch():
    for c in gf.CASES:
        n, h, w, ch, k, r, s, pad, g = c.geom
        assert ch % g == 0 and k % g == 0, c.id
        if c.entry in ("gfwd", "gdgrad_s1"):
            ctr, cols = (ch, k) if c.entry == "gfwd" else (k, ch)
            if ctr % 32 == 0 and cols % 4 == 0:
                assert c.form == ("sp2" if r * r * ctr > 1152 else "sp1"), c.id
            else:
                assert c.form == "f32", c.id
        elif c.entry == "gdgrad":
            assert c.form == "f32", c.id
            assert k % 16 == 0 and ch % 4 == 0 and s <= 8, c.id
        else:
            assert c.form == ("sp1" if ch % 4 == 0 and k % 4 == 0 else "f32"), c.id
            assert k % 4 == 0, c.id
        if c.entry == "gdgrad_s1":
            assert s == 1 and r - 1 - pad >= 0 and k % 16 == 0 and ch % 4 == 0 and c.opt.get("addend"), c.id      # ops.conv2d_dgrad's forward-kernel route


def test_only_the_depthwise_forward_goes_without_a_ratio_bar():
    free = [c for c in gf.CASES if c.opt.get("ratio_bar") is False]
    assert [c.branches for c in free] == [("gfwd.depthwise",)] and free[0].sparse and free[0].contracted_per_group == 1 and free[0].form == "sp1"
    assert 1.05 < gf.SPARSE_BANK_BAR <= 2.0 and gf.DENSE_BAR == 1.05
    # sparse = fewer than 32 contracted channels per group on a forward-kernel launch: 1, 4, 8, 24 here (16 is the K-step-16 case, fp32 MFMA only)
    assert sorted({c.contracted_per_group for c in gf.CASES if c.sparse and c.form != "f32"}) == [1, 4, 8, 24]


def _spans(c):
    return go.case_spans(c.entry, c.geom)


def test_the_restated_spans_show_what_the_labels_claim():
    def leaves_out(c):
        ncol, nctr, spans = _spans(c)
        return spans is not None and any(hi - lo < nctr for _, _, lo, hi in spans) and len({(lo, hi) for _, _, lo, hi in spans}) > 1

    for label in ("gfwd.span_bk32", "gfwd.span_rounded", "gfwd.span_bk16", "gfwd.spans_differ", "gfwd.taps5", "gfwd.depthwise", "gfwd.1x1", "gdgrad.s1_as_fwd",
                  "gdgrad.bk32", "gdgrad.bk16", "gdgrad.no_tap_classes", "gdgrad.stride1_entry", "gdgrad.stride3"):
        for c in BY_BRANCH[label]:
            if label == "gdgrad.s1_as_fwd" and c.geom[8] == 2:
                continue                                               # the straddle geometry: below
            assert leaves_out(c), (c.id, _spans(c)[2])
    # every span is whole k-steps inside the contraction, holds the channels of every group its columns belong to, and the listed spans of the issue
    for c in gf.CASES:
        if c.entry == "gwgrad":
            continue
        ncol, nctr, spans = _spans(c)
        if spans is None:
            continue
        per_col, per_ctr = ncol // c.geom[8], nctr // c.geom[8]
        bk = 32 if nctr % 32 == 0 else 16
        assert [n0 for n0, _, _, _ in spans] == list(range(0, ncol, 64))
        for n0, n1, lo, hi in spans:
            assert 0 <= lo < hi <= nctr and lo % bk == 0 and (hi - lo) % bk == 0, (c.id, n0, lo, hi)
            assert lo <= (n0 // per_col) * per_ctr and ((n1 - 1) // per_col + 1) * per_ctr <= hi, (c.id, n0, lo, hi)
            assert lo + bk > (n0 // per_col) * per_ctr and hi - bk < ((n1 - 1) // per_col + 1) * per_ctr, f"{c.id}: span wider than one k-step of rounding"
    want = {"gfwd.span_bk32": [[(0, 64), (64, 128)], [(0, 64), (64, 128), (128, 192), (192, 256)]],
            "gfwd.straddle": [[(0, 96), (0, 192), (96, 192)]], "gfwd.k_ragged": [[(0, 64), (32, 96), (64, 96)]], "gfwd.span_rounded": [[(0, 96), (32, 96)]],
            "gfwd.span_bk16": [[(0, 32), (32, 48)]], "gfwd.taps5": [[(0, 32), (32, 64)]], "gdgrad.bk16": [[(0, 32), (32, 48)]],
            "gdgrad.c_ragged": [[(0, 32), (16, 48), (32, 48)]], "gfwd.spans_differ": [[(0, 32), (32, 64), (64, 96), (96, 128)], [(0, 128), (128, 256)]]}
    for label, lists in want.items():
        assert [[(lo, hi) for _, _, lo, hi in _spans(c)[2]] for c in BY_BRANCH[label]] == lists, label
    # straddle: a tile that holds columns of two groups; ragged: a last tile of 4 columns; rounded: an edge that is no whole k-step before rounding
    for c in BY_BRANCH["gfwd.straddle"] + [c for c in BY_BRANCH["gdgrad.s1_as_fwd"] if c.geom[8] == 2]:
        ncol, nctr, spans = _spans(c)
        per_col = ncol // c.geom[8]
        assert any(n0 // per_col != (n1 - 1) // per_col for n0, n1, _, _ in spans), c.id
    for label in ("gfwd.k_ragged", "gdgrad.c_ragged"):
        for c in BY_BRANCH[label]:
            n0, n1, lo, hi = _spans(c)[2][-1]
            assert n1 - n0 == 4 and lo > 0, c.id
    (c,) = BY_BRANCH["gfwd.span_rounded"]
    cg = c.geom[3] // c.geom[8]
    assert any((n0 // (c.geom[4] // c.geom[8])) * cg % 32 for n0, _, _, _ in _spans(c)[2]) and any((((n1 - 1) // (c.geom[4] // c.geom[8])) + 1) * cg % 32 for _, n1, _, _ in _spans(c)[2])
    # the launches that ignore the groups
    for label in ("gfwd.dense_scalar", "gfwd.dense_c4", "gfwd.groups1"):
        for c in BY_BRANCH[label]:
            assert _spans(c)[2] is None, c.id
    # the poison test: a non-empty clean set and a non-empty complement
    for cid, groups in gf.POISON:
        c = gf.BY_ID[cid]
        for g in groups:
            clean = go.clean_columns(c.entry, c.geom, g)
            assert clean.any() and not clean.all(), (cid, g)


def test_the_restated_weight_gradient_plans_show_what_the_labels_claim():
    expect = {"gwgrad.bd_s1": (True, "s1", 18, 36), "gwgrad.bd_generic": (True, "generic", 108, 144), "gwgrad.bd_lin": (True, "lin", 2, 6),
              "gwgrad.bd_spans_differ": (True, "generic", 36, 72), "gwgrad.dense_tiles_skip": (False, "lin", 2, 4), "gwgrad.depthwise": (True, "s1", 18, 36)}
    for label, (bd, gather, nskip, ntiles) in expect.items():
        for c in BY_BRANCH[label]:
            p, tiles = go.WgradPlan(c.geom), go.wgrad_tiles(c.geom)
            assert (p.bd, p.gather) == (bd, gather), (c.id, p.bd, p.gather)
            assert (p.bm, p.bn_kernel) == ((64, 64) if bd else (128, 128)), c.id
            assert (sum(t[4] for t in tiles), len(tiles)) == (nskip, ntiles), (c.id, sum(t[4] for t in tiles), len(tiles))
    for c in BY_BRANCH["gwgrad.dense_tiles_noskip"]:
        p = go.WgradPlan(c.geom)
        assert not p.bd and p.bn_kernel == 128 and not any(t[4] for t in go.wgrad_tiles(c.geom)), c.id
        assert any(t[2] // c.geom[3] != (t[3] - 1) // c.geom[3] for t in go.wgrad_tiles(c.geom)), "no column tile straddles a tap"
    for c in BY_BRANCH["gwgrad.gbk"]:
        p = go.WgradPlan(c.geom)
        assert c.geom[3] % 4 != 0 and p.bn == 64 and p.bn_kernel == 128 and len(go.wgrad_tiles(c.geom)) == p.it * p.jt, c.id
    for c in BY_BRANCH["gwgrad.nsplit_ragged"]:
        p = go.WgradPlan(c.geom)
        assert p.chunks == [224, 224, 140], (c.id, p.chunks)
        assert p.nsplit >= 2 and p.chunks[-1] < p.chunk and any(t[4] for t in go.wgrad_tiles(c.geom))
    assert sorted(bool(c.opt.get("accumulate")) for c in BY_BRANCH["gwgrad.nsplit_ragged"]) == [False, True]
    assert all(c.opt.get("accumulate") for c in BY_BRANCH["gwgrad.accumulate"])
    for c in gf.CASES:
        if c.entry != "gwgrad":
            continue
        skipped, diag = go.skipped_mask(c.geom), go.diagonal_mask(c.geom)
        assert not (skipped & diag).any(), f"{c.id}: the restated rule skips a tile that a group touches"
        assert int(diag.sum()) == c.geom[4] * c.geom[5] ** 2 * (c.geom[3] // c.geom[8])
        tiles = go.wgrad_tiles(c.geom)
        assert len(tiles) == go.WgradPlan(c.geom).it * go.WgradPlan(c.geom).jt, f"{c.id}: the kernel's tiles are not the plan's grid"


def _desc(geom):
    n, h, w, c, k, r, s, pad, g = geom
    ho, wo = go.out_hw(geom)
    return _lib.ConvDesc(n, h, w, c, k, r, r, s, pad, ho, wo)


def test_the_restated_plan_is_the_librarys():
    lib = _lib.load()
    seen = 0
    for c in gf.CASES:
        n, h, w, ch, k, r, s, pad, g = c.geom
        d = _desc(c.geom)
        if c.entry == "gwgrad":
            p = go.WgradPlan(c.geom)
            assert p.workspace_bytes == p.nsplit * k * r * r * ch * 4
            assert int(lib.ssv_conv2d_wgrad_grouped_workspace_bytes(C.byref(d), g)) == p.workspace_bytes, c.id
            seen += 1
        assert int(lib.ssv_conv2d_wgrad_grouped_workspace_bytes(C.byref(d), 1)) == int(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d))), c.id
        assert go.WgradPlan(c.geom[:8] + (1,)).workspace_bytes == int(lib.ssv_conv2d_wgrad_workspace_bytes(C.byref(d))), c.id
    assert seen == 10
    q = lib.ssv_conv2d_wgrad_grouped_workspace_bytes
    d = _desc((2, 6, 6, 96, 96, 3, 1, 1, 3))
    assert q(None, 3) == 0 and q(C.byref(d), 0) == 0 and q(C.byref(d), -1) == 0 and q(C.byref(d), 5) == 0


@pytest.mark.parametrize("case", gf.CASES, ids=lambda c: c.id)
def test_the_references_are_conditioned(case):
    n, h, w, c, k, r, s, pad, g = case.geom
    t = gf.reference(case)
    ref, amag = t["ref"], t["amag"]
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    if case.entry == "gdgrad" and r == 1 and s == 2:                 # pixels of the three parity classes without a tap: exactly the addend (or zero)
        tapless = torch.ones(h, w, dtype=torch.bool)
        tapless[::2, ::2] = False
        base = torch.zeros_like(ref) if t["addend"] is None else t["addend"].double()
        assert torch.equal(ref[:, tapless], base[:, tapless]) and torch.equal(amag[:, tapless], base[:, tapless].abs())
        assert (amag[:, ~tapless] > 0).all()
    else:
        assert (amag > 0).all(), "A == 0 at a compared element"
    assert (ref.abs() <= amag * (1 + 1e-12)).all()
    # the grouped fp64 reference against the dense fp64 operation on the expanded bank: on the seeded operands to fp64 rounding (the two sum in different orders),
    # and EXACTLY on small-integer operands, whose sums are exact in any order - the block structure, the group order and the layout are the same
    x64, dy64, wg64 = t["x"].double(), t["dy"].double(), t["wg"].double()

    def both(x_, dy_, wg_):
        bank = go.expand_bank(wg_, g)
        if case.entry == "gfwd":
            return go.conv64(x_, wg_, s, pad, g), go.conv64(x_, bank, s, pad, 1)
        if case.entry in ("gdgrad_s1", "gdgrad"):
            return go.dgrad64(dy_, wg_, (n, h, w, c), s, pad, g), go.dgrad64(dy_, bank, (n, h, w, c), s, pad, 1)
        dense = go.wgrad64(x_, dy_, (k, r, r, c), s, pad, 1)
        return go.wgrad64(x_, dy_, (k, r, r, c // g), s, pad, g), dense[go.diagonal_mask(case.geom)].view(k, r, r, c // g)

    a, b = both(x64, dy64, wg64)
    ma, _ = both(x64.abs(), dy64.abs(), wg64.abs())
    assert ((a - b).abs() <= 2.0 ** -40 * ma + 1e-300).all()          # at most 2,304 terms, each sum within terms x 2^-53 x A of the true one
    ints = lambda v: torch.round(v * 4).clamp(-8, 8)      # noqa: E731
    a, b = both(ints(x64), ints(dy64), ints(wg64 * (r * r * max(c, k) // g) ** 0.5))
    assert a.abs().max() > 0 and torch.equal(a, b), "the grouped reference is not the dense operation on the expanded bank"
    assert torch.equal(t["bank"], go.expand_bank(t["wg"], g)) and t["bank"].dtype == torch.float32
