"""CPU: the fp64 oracle of the kNN label agreement (tests/knn_agreement_oracle.py), the case table of tests/test_gpu_knn_agreement.py held to the route
selection restated in Python, the single-swap detection property of the labelling family, and the proof - in fp64 only - that the fp32 cases of the GPU file
meet the conditions under which their windows mean something (so whatever keeps a count inside its window is the kernel, not the data)."""
import os
import re

import numpy as np
import pytest

import knn_agreement_oracle as ko
import knn_classify_oracle as kc
import test_gpu_knn_agreement as gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "evalknn.hip")


# ====================================================================================================================== the oracle itself
def _brute(z, lab, k):
    """The definition, one query at a time on whole sorted rows."""
    s = kc.similarities(z, z)
    total = 0
    for q, row in enumerate(kc.order(s)):
        for j in row[1:k + 1]:
            if not np.isnan(s[q, j]):
                total += int(lab[j] == lab[q])
    return total


@pytest.mark.parametrize("family,n,d,k", [("ints", 130, 32, 20), ("tern", 97, 32, 7), ("ones", 40, 8, 39), ("dups", 90, 16, 1), ("nan", 60, 32, 59), ("zero_row", 50, 12, 20),
                                         ("blobs", 120, 36, 20)])
def test_lists_equal_whole_row_sorting(family, n, d, k):
    z = gpu.features(family, n, d, 0)
    idx = ko.lists(z, k)
    s = kc.similarities(z, z)
    whole = kc.order(s)[:, 1:k + 1]
    assert np.array_equal(np.where(idx < 0, whole, idx), whole)
    assert np.array_equal(idx < 0, np.isnan(np.take_along_axis(s, whole, axis=1)))
    for name, lab in ko.labelings(n):
        assert ko.expected(z, lab, k, idx) == _brute(z, lab, k), name


def test_order_and_nan_rules():
    z = np.array([[1, 0], [1, 0], [0, 1], [2, 0], [0, np.nan]], np.float32)
    idx = ko.lists(z, 2)
    # query 0: scores 1 1 0 2 NaN -> order 3 0 1 2 | 4: rank 0 (row 3, not the query) dropped
    assert idx.tolist() == [[0, 1], [0, 1], [0, 1], [0, 1], [-1, -1]]
    assert ko.lists(z, 4)[0].tolist() == [0, 1, 2, -1]                               # the NaN row is never a neighbour
    assert ko.expected(z, np.zeros(5, np.int32), 4) == 4 * 3                         # and the NaN query contributes nothing
    zero = np.array([[3, 1], [0, 0], [1, 1], [-1, 2]], np.float32)
    assert ko.lists(zero, 2)[1].tolist() == [1, 2]                                   # an all-zero query: every score ties, index 0 is dropped


def test_labelings_family():
    for n in (21, 300, 4100):
        labs = ko.labelings(n)
        planes = sum(1 for b in range(32) if (1 << b) < n)
        assert len(labs) == 2 + planes + 16 and len({name for name, _ in labs}) == len(labs)
        assert all(lab.dtype == np.int32 and lab.shape == (n,) and lab.min() >= 0 for _, lab in labs)
        assert (labs[0][1] == 0).all() and len(set(labs[1][1].tolist())) == n
    assert len(ko.labelings(300)) == 27
    assert ko.labelings(300) is ko.labelings(300)                                    # computed once, shared and read-only
    with pytest.raises(ValueError):
        ko.labelings(300)[0][1][0] = 1


def test_single_swap_of_rank_k_for_rank_k_plus_1_moves_a_count():
    """The integer case the GPU file ships at n 300, d 32 (padded from 30), k 20: each of the 300 single swaps changes at least one of the 27 counts."""
    case = next(c for c in gpu.CASES if c.family == "ints" and c.n == 300 and gpu.padded(c.d) == 32 and c.k == 20)
    z = gpu.case_features(case)
    n, k = case.n, case.k
    idx = ko.lists(z, k + 1)
    assert (idx >= 0).all()
    labs = ko.labelings(n)
    assert len(labs) == 27
    base = [ko.count(idx[:, :k], lab) for _, lab in labs]
    for q in range(n):
        swapped = idx[:, :k].copy()
        swapped[q, k - 1] = idx[q, k]
        moved = [ko.count(swapped, lab) != b for (_, lab), b in zip(labs, base)]
        assert any(moved), q
        assert any(m for m, (name, _) in zip(moved, labs) if name.startswith("bit")), q


def test_window_contains_the_exact_count_and_closes_on_clear_margins():
    z = gpu.features("blobs", 700, 36, 0)
    m = ko.margins(z, 7)
    idx = ko.lists(z, 7)
    for _, lab in ko.labelings(700):
        lo, hi, share = ko.window(z, lab, 7, m)
        assert lo <= ko.count(idx, lab) <= hi and share == m.excused_share
    lo, hi, _ = ko.window(z, ko.labelings(700)[0][1], 7, m)
    assert lo == hi == 700 * 7
    # exact scores with ties across rank k: every tie group is uncertain, and the window still holds the tie rule's count
    zi = gpu.features("tern", 97, 32, 0)
    mi = ko.margins(zi, 7)
    assert mi.excused_share > 0.5
    for _, lab in ko.labelings(97):
        lo, hi, _ = ko.window(zi, lab, 7, mi)
        assert lo <= ko.expected(zi, lab, 7) <= hi


def test_tau_is_the_conv_forms_rule():
    text = open(os.path.join(ROOT, "tests", "test_gpu_conv_forms.py")).read()
    fwd = re.search(r'TAU = \{"fwd": ([0-9.]+)', text)
    assert fwd and float(fwd.group(1)) == ko.TAU_FWD == 16.0
    assert ko.MAX_EXCUSED == kc.MAX_EXCUSED == 0.01 and ko.MAX_WIDTH == 2


# ====================================================================================================================== the case table
def test_case_table_covers_every_documented_branch():
    """Every branch label of the GPU file's docstring is named by a case, every case claims exactly the labels the restated selection gives it, ids are unique."""
    doc = gpu.documented_labels()
    assert len(doc) == 17, sorted(doc)
    used = {b for c in gpu.CASES for b in c.labels}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    for c in gpu.CASES:
        assert set(c.labels) == gpu.reaches(c.arith, c.d, c.n, c.k), (c.id, sorted(gpu.reaches(c.arith, c.d, c.n, c.k)))
        assert c.labels[0].split(".")[0] in ("fused", "unfused", "fallback"), c.id            # the route label first
        assert c.family in gpu.EXACT_FAMILIES + gpu.FP32_FAMILIES
    ids = [c.id for c in gpu.CASES]
    assert len(ids) == len(set(ids))
    src = open(SRC).read()
    for kernel in set(doc.values()) - {"ops.knn_label_agreement", "sp_fwd_ok"}:
        assert kernel.split("<")[0] in src, kernel


def test_restated_selection_reads_what_the_source_reads():
    """The predicates of ssv_knn_label_agreement_arith, choose_parts and knn_agree_k that gpu.reaches() restates, pinned to the text of csrc/evalknn.hip."""
    src = open(SRC).read()
    for needle in ("d % 32 != 0 || (n * d) % 8 != 0", "(d == 32 || d == 64 || d == 128) && k < fused::KEEP", "constexpr int KEEP = 21", "if (k <= 20)", "if (r > 4096) r = 4096",
                   "2 * (int64_t)cus / cdiv64(n, 128)", "cdiv64(n, p) < 32 * 8", "p > 8 ? 8 : p", "cdiv64(cdiv64(n, parts), 32) * 32", "(lds & 3) == 0", "n & ~1023", "n & ~511",
                   "k >= 1 && k <= 63 && k < n"):
        assert needle in src, needle
    conv = open(os.path.join(os.path.dirname(SRC), "conv_mfma.hip")).read()
    assert re.search(r"inline bool sp_fwd_ok[^}]*d->K % 4 == 0", conv)
    # a few answers by hand
    assert gpu.choose_parts(21, 256) == (1, 32) and gpu.choose_parts(129, 256) == (1, 160)
    assert gpu.choose_parts(700, 256) == (2, 352) and gpu.choose_parts(1000, 256) == (3, 352) and gpu.choose_parts(4100, 256) == (8, 544)
    assert [(n - (p - 1) * cpp) % 32 for n in (700, 1000, 4100) for p, cpp in (gpu.choose_parts(n, 256),)] == [28, 8, 4]      # valid columns of the last tile
    assert gpu.reaches("bf16x3", 512, 600, 20) == {"unfused.sp.cap21", "agree.loop512", "agree.tail"}                             # what build_features hands over
    assert gpu.reaches("bf16x3", 2048, 300, 20) == gpu.reaches("bf16x3", 384, 300, 20) == {"unfused.sp.cap21", "agree.tail"}
    assert gpu.reaches("bf16x3", 16, 300, 20) == gpu.reaches("bf16x3", 36, 300, 20) == {"fallback.f32", "agree.tail"}
    assert "fused.padded" in gpu.reaches("bf16x3", 126, 129, 20) and "fused.d128" in gpu.reaches("bf16x3", 126, 129, 20)
    assert "unfused.sp.cap64" in gpu.reaches("bf16x3", 128, 300, 21) and "fused.d128" in gpu.reaches("bf16x3", 128, 300, 20)


def test_the_table_holds_the_shapes_each_route_needs():
    by = lambda pred: [c for c in gpu.CASES if pred(c)]
    for d in (32, 64, 128):
        ns = {c.n for c in by(lambda c: c.labels[0] == f"fused.d{d}" and c.family == "ints")}
        assert {21, 129, 700, 1000, 4100} <= ns, (d, ns)
    assert any(c.n == 12000 and c.labels[0] == "fused.d32" for c in gpu.CASES)
    assert {c.d for c in by(lambda c: "fused.padded" in c.labels)} == {30, 126}
    assert {300, 1003, 1540, 4100, 4101} <= {c.n for c in by(lambda c: c.labels[0] == "unfused.sp.cap21")}
    assert {96, 256, 512} <= {c.d for c in by(lambda c: c.labels[0] == "unfused.sp.cap21")}
    assert {(65, 63), (1000, 21), (1000, 40), (4100, 21), (4100, 63)} <= {(c.n, c.k) for c in by(lambda c: c.labels[0] == "unfused.sp.cap64")}
    assert {36, 128, 512} <= {c.d for c in by(lambda c: c.labels[0].startswith("unfused.f32"))}
    assert {12, 36} <= {c.d for c in by(lambda c: c.labels[0] == "fallback.f32")}
    for fam in gpu.EXACT_FAMILIES[1:]:                                             # every content family on a fused, an unfused bf16x3 and an f32 route
        routes = {c.labels[0].rsplit(".", 1)[0] for c in by(lambda c: c.family == fam)}
        assert {"fused", "unfused.sp", "unfused.f32"} <= routes, (fam, routes)
    for k_rule in (lambda c: c.k == 1, lambda c: c.k == c.n - 1):
        routes = {c.labels[0].rsplit(".", 1)[0] for c in by(k_rule)}
        assert {"fused", "unfused.sp", "unfused.f32"} <= routes, routes
    for fam in gpu.FP32_FAMILIES:
        assert {c.arith for c in by(lambda c: c.family == fam)} == set(gpu.ARITHMETICS)
    fp32_routes = {c.labels[0] for c in gpu.FP32_CASES}
    assert {"fused.d32", "fused.d64", "fused.d128", "unfused.sp.cap21", "unfused.sp.cap64", "unfused.f32.cap21", "unfused.f32.cap64", "fallback.f32"} <= fp32_routes


# ====================================================================================================================== the exact cases' inputs
def test_exact_families_are_exact_and_do_what_their_names_say():
    for c in gpu.CONTENT_CASES + gpu.ROUTE_CASES[:3]:
        z = gpu.case_features(c).astype(np.float64)
        ok = ~np.isnan(z).any(1)
        assert np.array_equal(z[ok], np.round(z[ok])), c.id
        za = np.abs(z[ok])
        assert np.abs(z[ok]).max() < 2 ** 16                                       # at most two bf16 pieces: every kept piece product is exact
        mag = za @ za.T
        off = mag[~np.eye(mag.shape[0], dtype=bool)]
        assert off.max() < 2 ** 24, c.id                                           # every partial sum of every score that can decide a rank is exact in fp32
        if c.family != "negq":
            assert mag.max() < 2 ** 24, c.id
    n, k = 700, 20
    s = ko.scores(gpu.features("tern", n, 32, 0))
    share = float(kc.straddling_ties(s, k + 1).mean())                              # ranks 0 .. k are kept: the value at rank k also occurs at rank k + 1
    assert share > 0.5, share
    s = ko.scores(gpu.features("negq", n, 32, 0))
    q = n // 2
    assert (np.delete(s[q], q) < 0).all() and s[q, q] > 0 and (np.delete(s[:, q], q) < 0).all()
    z = gpu.features("ints300", n, 32, 0)
    import torch
    hi = torch.tensor(z).bfloat16().float().numpy()
    assert float((hi != z).mean()) > 0.05                                          # the odd values above 256 need a second bf16 piece (every row holds some) ...
    assert (hi != z).any(1).mean() > 0.8
    assert np.array_equal(torch.tensor(z - hi).bfloat16().float().numpy(), z - hi)  # ... and none needs a third
    z = gpu.features("dups", n, 32, 0)
    assert np.array_equal(z[:234], z[234:468]) and np.array_equal(z[:232], z[468:])
    assert not gpu.features("zero_row", n, 32, 0)[n // 3].any()
    for c in (c for c in gpu.CASES if c.family == "lane"):                         # the tie group at the top of a special row is deeper than a lane's list
        z, s = gpu.case_features(c), ko.scores(gpu.case_features(c), 5, 6)[0]
        tied = np.flatnonzero(s == s.max())
        assert len(tied) > (21 if c.k <= 20 else 64) and (tied % 64 == 5).all() and ko.lists(z, c.k)[5].tolist() == tied[1:c.k + 1].tolist(), c.id
    assert np.isnan(gpu.features("nan", n, 32, 0)).sum() == 1
    # the dropped hit is not always the query: ones (index 0 for everybody) and the unnormalised families
    assert (kc.order(ko.scores(gpu.features("ones", 40, 8, 0)))[:, 0] == 0).all()


# ====================================================================================================================== the fp32 cases' conditions
@pytest.mark.parametrize("shape", gpu.FP32_SHAPES, ids=lambda s: "%s-n%d-d%d-k%d" % s[:4])
def test_fp32_cases_meet_the_conditions_of_their_windows(shape):
    """Conditions, not measurements: excused share <= 1 %, no query with its two best scores within 2 tau (an ambiguous dropped hit), hi - lo <= 2 for every
    labelling - from the fp64 reference alone."""
    family, n, d, k, seed = shape[:5]
    z = gpu.features(family, n, d, seed)
    m = gpu.case_margins(family, n, d, k, seed)
    widths = []
    for _, lab in ko.labelings(n):
        lo, hi, _ = ko.window(z, lab, k, m)
        widths.append(hi - lo)
    own = float((kc.order(ko.scores(z, 0, 256))[:, 0] == np.arange(min(256, n))).mean())
    print(f"{family} {n} x {d}, k {k}: excused {m.excused_share:.2%}, ambiguous dropped hits {int(m.ambiguous.sum())}, widest window {max(widths)}, "
          f"dropped hit is the query for {own:.0%} of the first rows")
    assert m.excused_share <= ko.MAX_EXCUSED
    assert not m.ambiguous.any()
    assert max(widths) <= ko.MAX_WIDTH
    if family == "relu":
        assert own < 0.5                                                           # mostly NOT the query itself
