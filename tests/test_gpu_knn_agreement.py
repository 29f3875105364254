"""GPU: the kNN label agreement (ssv_knn_label_agreement_arith, csrc/evalknn.hip) on every route, neighbour by neighbour, against the fp64 lists of
tests/knn_agreement_oracle.py.

Every case runs the DIRECT C-ABI call into guarded buffers: `count` is one word prefilled with a non-zero pattern and 64 sentinel words behind it, the workspace
is what ssv_knn_workspace_bytes_arith answers for the arithmetic asked for with 1024 sentinel bytes behind it, the feature matrix and the labels stand in front
of sentinels of their own and are compared bit for bit afterwards.  One call per labelling of knn_agreement_oracle.labelings (all equal, all distinct, the bit
planes of the index, 16 random ones - the features are uploaded once, only the labels change), a second identical call that must return the same count, and
ops.knn_label_agreement once, which must return what the ABI did.

Exact cases (integer-valued features: every score is exact in both arithmetics, so the lists ARE the oracle's, tie rule included): count == expected for every
labelling.  fp32 features (unit-length blobs, unnormalised post-ReLU features): lo <= count <= hi for every labelling, the window of knn_agreement_oracle.window
with tau_q = 16 * 2^-24 * max_j sum_c |z_qc| |z_jc| (rule (a) of tests/test_gpu_conv_forms.py, TAU["fwd"]).  tests/test_knn_agreement_cpu.py proves on the CPU
that at most 1 % of the queries of each such case are excused, that no dropped hit is ambiguous and that no window is wider than 2 - so a count outside its
window is a finding about the kernel; nothing here is measured from it.

Branch labels (label, the kernel or host line that decides, what the case reaches) - tests/test_knn_agreement_cpu.py::test_case_table_covers_every_documented_branch
restates the selection of ssv_knn_label_agreement_arith, choose_parts and knn_agree_k's loops in Python and holds every case to the labels it claims:

  fused.d32            knn_fused_k<32>               bf16x3, d 32, k <= 20
  fused.d64            knn_fused_k<64>               bf16x3, d 64, k <= 20
  fused.d128           knn_fused_k<128>              bf16x3, d 128, k <= 20
  fused.padded         ops.knn_label_agreement       d 30 -> 32 and 126 -> 128: ops pads with zero columns (the ABI call gets the padded matrix)
  fused.parts1         choose_parts                  one column part on a 256-CU device (n 21: under one wave of queries, k = n - 1; n 129: the second workgroup holds one query)
  fused.partsN         choose_parts                  2, 3 and 8 column parts on a 256-CU device (n 700, 1000, 4100: last tiles of 28, 8 and 4 valid columns; n 12000)
  unfused.sp.cap21     knn_agree_k<21>               bf16x3, d % 32 == 0 outside {32, 64, 128}, k <= 20: ssv_split_planes into the workspace's tail, the product with w_planes
  unfused.sp.cap64     knn_agree_k<64>               bf16x3, d % 32 == 0, 21 <= k <= 63
  unfused.f32.cap21    knn_agree_k<21>               "f32" asked for, k <= 20
  unfused.f32.cap64    knn_agree_k<64>               "f32" asked for, k >= 21
  fallback.f32         ssv_knn_label_agreement_arith  bf16x3 asked for at d % 32 != 0 (36, 12): no piece kernel; the count is bit-identical to the "f32" run's
  agree.tail           knn_agree_k                   n % 4 == 0 and n % 512 != 0: the one-column-per-lane tail behind the vector loops (n 300: the tail alone)
  agree.loop512        knn_agree_k                   n % 4 == 0 and n % 1024 >= 512: the 512-column loop (n 1000, 1540)
  agree.loop1024       knn_agree_k                   n % 4 == 0 and n >= 1024: the 1024-column loop (n 1540: all three loops in one row)
  agree.scalar         knn_agree_k                   n % 4 != 0 (n 1003, 4101): rows of S are not 16-byte aligned, the scalar path alone
  agree.chunks2        chunk_rows                    n > 4096: two row chunks (4096 and 4 rows at n 4100: a last workgroup with empty waves)
  gram.k_mod4          sp_fwd_ok                     bf16x3 on the unfused route with n % 4 != 0: the planes are split, the product itself runs on fp32 MFMA

Under SSV_KNN_AGREE_REPORT=<path> the file writes route, part count, counts, windows and excused share per case and the library's source_sha16
(profiles/knn_agreement_report.json is that file from an MI355X)."""
import collections
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import knn_agreement_oracle as ko

pytestmark = pytest.mark.gpu
ARITHMETICS = ("bf16x3", "f32")
COUNT_PATTERN = 0x5A5A5A5A5A5A5A5A
COUNT_GUARD = 64                     # words behind count
WS_GUARD = 1024                      # bytes behind the workspace
WS_FILL = 0xA5
IN_GUARD = 64                        # words behind z and behind the labels (-1: matches no label)
REPORT = {}

Case = collections.namedtuple("Case", "id arith family n d k seed labels")


def _c(arith, family, n, d, k, labels, seed=0):
    return Case(f"{family}-{arith}-n{n}-d{d}-k{k}", arith, family, n, d, k, seed, tuple(labels.split()))


EXACT_FAMILIES = ("ints", "ints300", "ones", "tern", "dups", "zero_row", "negq", "nan", "lane")
FP32_FAMILIES = ("blobs", "blobs200", "relu")

# ---- routes: small integers in {-2 .. 2}
ROUTE_CASES = tuple(
    [_c("bf16x3", "ints", n, d, k, f"fused.d{d} {parts}") for d in (32, 64, 128)
     for n, k, parts in ((21, 20, "fused.parts1"), (129, 20, "fused.parts1"), (700, 20, "fused.partsN"), (1000, 7, "fused.partsN"), (4100, 20, "fused.partsN"))]
    + [_c("bf16x3", "ints", 12000, 32, 20, "fused.d32 fused.partsN"),
       _c("bf16x3", "ints", 300, 30, 20, "fused.d32 fused.padded fused.parts1"),
       _c("bf16x3", "ints", 129, 126, 20, "fused.d128 fused.padded fused.parts1"),
       _c("bf16x3", "ints", 300, 96, 20, "unfused.sp.cap21 agree.tail"),
       _c("bf16x3", "ints", 1003, 256, 20, "unfused.sp.cap21 agree.scalar gram.k_mod4"),
       _c("bf16x3", "ints", 1540, 512, 20, "unfused.sp.cap21 agree.loop1024 agree.loop512 agree.tail"),
       _c("bf16x3", "ints", 1000, 512, 7, "unfused.sp.cap21 agree.loop512 agree.tail"),
       _c("bf16x3", "ints", 4100, 96, 20, "unfused.sp.cap21 agree.chunks2 agree.loop1024 agree.tail"),
       _c("bf16x3", "ints", 4101, 96, 20, "unfused.sp.cap21 agree.chunks2 agree.scalar gram.k_mod4"),
       _c("bf16x3", "ints", 65, 128, 63, "unfused.sp.cap64 agree.scalar gram.k_mod4"),
       _c("bf16x3", "ints", 1000, 96, 21, "unfused.sp.cap64 agree.loop512 agree.tail"),
       _c("bf16x3", "ints", 1000, 128, 40, "unfused.sp.cap64 agree.loop512 agree.tail"),
       _c("bf16x3", "ints", 4100, 128, 21, "unfused.sp.cap64 agree.chunks2 agree.loop1024 agree.tail"),
       _c("bf16x3", "ints", 4100, 96, 63, "unfused.sp.cap64 agree.chunks2 agree.loop1024 agree.tail"),
       _c("f32", "ints", 300, 128, 20, "unfused.f32.cap21 agree.tail"),
       _c("f32", "ints", 1003, 512, 20, "unfused.f32.cap21 agree.scalar"),
       _c("f32", "ints", 1540, 36, 20, "unfused.f32.cap21 agree.loop1024 agree.loop512 agree.tail"),
       _c("f32", "ints", 4100, 128, 20, "unfused.f32.cap21 agree.chunks2 agree.loop1024 agree.tail"),
       _c("f32", "ints", 65, 128, 63, "unfused.f32.cap64 agree.scalar"),
       _c("f32", "ints", 1000, 36, 40, "unfused.f32.cap64 agree.loop512 agree.tail"),
       _c("f32", "ints", 4100, 512, 21, "unfused.f32.cap64 agree.chunks2 agree.loop1024 agree.tail"),
       _c("bf16x3", "ints", 1000, 36, 20, "fallback.f32 agree.loop512 agree.tail"),
       _c("bf16x3", "ints", 300, 12, 7, "fallback.f32 agree.tail"),
       _c("bf16x3", "ints", 1000, 36, 40, "fallback.f32 agree.loop512 agree.tail")])

# ---- content: each on one fused route, one unfused bf16x3 route and one f32 route (n 700: two column parts on a 256-CU device)
_FUSED32, _SP32, _SP96, _F32 = ("bf16x3", 32, 20, "fused.d32 fused.partsN"), ("bf16x3", 32, 21, "unfused.sp.cap64 agree.loop512 agree.tail"), \
    ("bf16x3", 96, 20, "unfused.sp.cap21 agree.loop512 agree.tail"), ("f32", 32, 20, "unfused.f32.cap21 agree.loop512 agree.tail")
CONTENT_CASES = tuple(
    [_c(a, fam, 700, d, k, lab) for fam, routes in (("ones", (_FUSED32, _SP96, _F32)), ("tern", (_FUSED32, _SP32, _F32)), ("dups", (_FUSED32, _SP96, _F32)),
                                                    ("zero_row", (_FUSED32, _SP96, _F32)), ("ints300", (_FUSED32, _SP32, _F32)), ("negq", (_FUSED32, _SP96, _F32)),
                                                    ("nan", (_FUSED32, _SP96, _F32)))
     for a, d, k, lab in routes]
    # one LANE of knn_agree_k's scalar path (column j goes to lane j % 64) meets more tied best scores than its private list holds: 32 and 80 equal rows
    + [_c("bf16x3", "lane", 2049, 32, 20, "fused.d32 fused.partsN"),
       _c("bf16x3", "lane", 2049, 96, 20, "unfused.sp.cap21 agree.scalar gram.k_mod4"),
       _c("f32", "lane", 2049, 36, 20, "unfused.f32.cap21 agree.scalar"),
       _c("f32", "lane", 5121, 36, 63, "unfused.f32.cap64 agree.chunks2 agree.scalar")]
    + [_c("bf16x3", "ints", 700, 64, 1, "fused.d64 fused.partsN", seed=1),                       # k = 1
       _c("bf16x3", "ints", 700, 96, 1, "unfused.sp.cap21 agree.loop512 agree.tail", seed=1),
       _c("f32", "ints", 700, 64, 1, "unfused.f32.cap21 agree.loop512 agree.tail", seed=1),
       _c("bf16x3", "ints", 21, 96, 20, "unfused.sp.cap21 agree.scalar gram.k_mod4", seed=1),                  # k = n - 1 (fused: n 21 above)
       _c("f32", "ints", 21, 32, 20, "unfused.f32.cap21 agree.scalar", seed=1),
       _c("bf16x3", "ints", 64, 128, 63, "unfused.sp.cap64 agree.tail", seed=1),
       _c("f32", "ints", 64, 128, 63, "unfused.f32.cap64 agree.tail", seed=1)])

# ---- fp32 features, each shape under both arithmetics: (family, n, d, k, seed, labels under bf16x3, labels under f32).  Seeds and class counts are those at
# which the fp64 reference ALONE meets the conditions of tests/test_knn_agreement_cpu.py (excused share, no ambiguous dropped hit, window width)
FP32_SHAPES = (
    ("blobs", 1500, 128, 20, 0, "fused.d128 fused.partsN", "unfused.f32.cap21 agree.loop1024 agree.tail"),
    ("blobs", 1200, 96, 20, 0, "unfused.sp.cap21 agree.loop1024 agree.tail", "unfused.f32.cap21 agree.loop1024 agree.tail"),
    ("blobs", 1000, 64, 40, 0, "unfused.sp.cap64 agree.loop512 agree.tail", "unfused.f32.cap64 agree.loop512 agree.tail"),
    ("blobs", 1000, 64, 20, 0, "fused.d64 fused.partsN", "unfused.f32.cap21 agree.loop512 agree.tail"),
    ("blobs", 700, 36, 7, 0, "fallback.f32 agree.loop512 agree.tail", "unfused.f32.cap21 agree.loop512 agree.tail"),
    ("blobs200", 4500, 32, 20, 0, "fused.d32 fused.partsN", "unfused.f32.cap21 agree.chunks2 agree.loop1024 agree.tail"),
    ("blobs", 1100, 256, 20, 0, "unfused.sp.cap21 agree.loop1024 agree.tail", "unfused.f32.cap21 agree.loop1024 agree.tail"),
    ("relu", 600, 512, 20, 0, "unfused.sp.cap21 agree.loop512 agree.tail", "unfused.f32.cap21 agree.loop512 agree.tail"),
    ("relu", 500, 384, 20, 0, "unfused.sp.cap21 agree.tail", "unfused.f32.cap21 agree.tail"),
    ("relu", 4100, 96, 20, 8, "unfused.sp.cap21 agree.chunks2 agree.loop1024 agree.tail", "unfused.f32.cap21 agree.chunks2 agree.loop1024 agree.tail"),
)
FP32_CASES = tuple(_c(a, fam, n, d, k, lab, seed) for fam, n, d, k, seed, lb, lf in FP32_SHAPES for a, lab in (("bf16x3", lb), ("f32", lf)))
CASES = ROUTE_CASES + CONTENT_CASES + FP32_CASES


# ====================================================================================================================== the selection, restated
def padded(d):
    return (d + 3) // 4 * 4


def cdiv(a, b):
    return -(-a // b)


def choose_parts(n, cus):
    """fused::choose_parts and the rounding of ssv_knn_label_agreement_arith behind it: (parts, columns per part)."""
    p = 2 * cus // cdiv(n, 128)
    while p > 1 and cdiv(n, p) < 32 * 8:
        p -= 1
    p = min(max(p, 1), 8)
    cpp = cdiv(cdiv(n, p), 32) * 32
    return cdiv(n, cpp), cpp


def reaches(arith, d_raw, n, k, cus=256):
    """The labels a call reaches, from the predicates the selection reads: d % 32, (n d) % 8, d in {32, 64, 128}, k < 21 - and below them the loops of knn_agree_k."""
    d = padded(d_raw)
    assert 2 <= n and 1 <= k <= min(63, n - 1)
    out = set()
    fell_back = arith == "bf16x3" and (d % 32 != 0 or (n * d) % 8 != 0)
    pieces = arith == "bf16x3" and not fell_back
    if pieces and d in (32, 64, 128) and k < 21:
        out.add(f"fused.d{d}")
        out.add("fused.parts1" if choose_parts(n, cus)[0] == 1 else "fused.partsN")
        if d != d_raw:
            out.add("fused.padded")
        return out
    cap = "cap21" if k <= 20 else "cap64"
    out.add("fallback.f32" if fell_back else f"unfused.sp.{cap}" if pieces else f"unfused.f32.{cap}")
    if pieces and n % 4 != 0:
        out.add("gram.k_mod4")
    if n > 4096:
        out.add("agree.chunks2")
    if n % 4 != 0:
        out.add("agree.scalar")
    else:
        if n >= 1024:
            out.add("agree.loop1024")
        if n % 1024 >= 512:
            out.add("agree.loop512")
        if n % 512 != 0:
            out.add("agree.tail")
    return out


def documented_labels():
    """{label: deciding kernel} from the Branch labels block of the module docstring."""
    block = __doc__.split("Branch labels", 1)[1].split("Under SSV_KNN_AGREE_REPORT", 1)[0]
    return dict(re.findall(r"^  ([a-z0-9_.A-Z]+)\s{2,}(\S+)\s{2,}\S", block, re.M))


# ====================================================================================================================== inputs and expectations
@functools.lru_cache(maxsize=None)
def features(family, n, d, seed):
    """[n, d] fp32, read-only; drawn on the CPU from the case's seed."""
    if family == "ints":
        z = ko.small_ints(n, d, seed)
    elif family == "ints300":                               # two bf16 pieces per value
        z = ko.two_piece_ints(n, seed, d)
    elif family == "ones":                                  # every score equal: the lowest indices win, the dropped hit is index 0
        z = np.ones((n, d), np.float32)
    elif family == "tern":                                  # {-1, 0, 1}: ties straddle rank k for most queries
        z = ko.small_ints(n, d, 200 + seed, -1, 1)
    elif family == "dups":                                  # every row three times
        z = ko.small_ints(n, d, 300 + seed)
        z = z[np.arange(n) % cdiv(n, 3)].copy()
    elif family == "zero_row":
        z = ko.small_ints(n, d, 400 + seed)
        z[n // 3] = 0.0
    elif family == "negq":                                  # one query is minus the sum of the other (positive) rows: every other score of it is negative
        z = ko.small_ints(n, d, 500 + seed, 1, 5)
        q = n // 2
        z[q] = -(z.sum(0) - z[q])
    elif family == "nan":                                   # the LAST row: the one the fused kernel's clamped loads repeat
        z = ko.small_ints(n, d, 600 + seed)
        z[n - 1, 5] = np.nan
    elif family == "lane":                                  # rows 5, 69, 133, ... are one vector of threes: tied at the top of their own rows, all in lane 5
        z = ko.small_ints(n, d, 700 + seed)
        z[5::64] = 3.0
    elif family == "blobs":
        z = ko.blob_features(n, d, seed)
    elif family == "blobs200":                              # 200 classes: at n 4500 fewer near-ties at rank k than ten crowded classes give
        z = ko.blob_features(n, d, seed, classes=200)
    elif family == "relu":
        z = ko.relu_features(n, d, seed)
    else:
        raise KeyError(family)
    z = np.ascontiguousarray(z, np.float32)
    z.setflags(write=False)
    return z


def case_features(c):
    return features(c.family, c.n, c.d, c.seed)


@functools.lru_cache(maxsize=None)
def neighbour_lists(family, n, d, k, seed):
    return ko.lists(features(family, n, d, seed), k)


@functools.lru_cache(maxsize=None)
def case_margins(family, n, d, k, seed):
    return ko.margins(features(family, n, d, seed), k)


# ====================================================================================================================== the guarded call
def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


class Guarded:
    """Device buffers of one case: z and the labels in front of IN_GUARD sentinel words, count in front of COUNT_GUARD pattern words, the workspace of
    ssv_knn_workspace_bytes_arith(n, d, arithmetic asked for) bytes in front of WS_GUARD bytes of WS_FILL."""

    def __init__(self, z, arith):
        from ssv_amd import _lib
        self.n, d_raw = z.shape
        self.d = padded(d_raw)
        zp = np.zeros((self.n, self.d), np.float32)
        zp[:, :d_raw] = z                                   # what ops.knn_label_agreement hands over: zero columns
        self.code = _code(arith)
        self.zbuf = torch.full((self.n * self.d + IN_GUARD,), 12345.0, device="cuda")
        self.zbuf[:self.n * self.d] = torch.from_numpy(zp.reshape(-1)).cuda()
        self.zkeep = self.zbuf.clone()
        self.lbuf = torch.full((self.n + IN_GUARD,), -1, dtype=torch.int32, device="cuda")
        self.cbuf = torch.empty(1 + COUNT_GUARD, dtype=torch.int64, device="cuda")
        self.ws_bytes = int(_lib.load().ssv_knn_workspace_bytes_arith(self.n, self.d, self.code))
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes + WS_GUARD, dtype=torch.uint8, device="cuda")
        self.ws.fill_(WS_FILL)
        assert self.zbuf.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0

    def set_labels(self, lab):
        self.lbuf[:self.n] = torch.tensor(np.asarray(lab, np.int32)).cuda()
        self.lkeep = self.lbuf.clone()

    def raw(self, k, n=None, d=None, z_off=0, ws_bytes=None):
        """The return code of the entry point itself; count is re-armed with the pattern first."""
        from ssv_amd import _lib
        self.cbuf.fill_(COUNT_PATTERN)
        rc = _lib.load().ssv_knn_label_agreement_arith(self.n if n is None else n, self.d if d is None else d, self.zbuf.data_ptr() + z_off, self.lbuf.data_ptr(), k,
                                                       self.cbuf.data_ptr(), self.code, self.ws.data_ptr(), self.ws_bytes if ws_bytes is None else ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        return rc

    def check_untouched(self, what):
        assert torch.equal(self.zbuf.view(torch.int32), self.zkeep.view(torch.int32)), f"{what}: the features (or their guard) were modified"
        assert torch.equal(self.lbuf, self.lkeep), f"{what}: the labels (or their guard) were modified"
        assert bool((self.cbuf[1:] == COUNT_PATTERN).all()), f"{what}: wrote behind count"
        assert bool((self.ws[self.ws_bytes:] == WS_FILL).all()), f"{what}: wrote behind the workspace ssv_knn_workspace_bytes_arith asked for"

    def count(self, k):
        from ssv_amd import _lib
        rc = self.raw(k)
        assert rc == 0, (rc, _lib.load().ssv_last_error())
        self.check_untouched("call")
        got = int(self.cbuf[0].item())
        assert got != COUNT_PATTERN, "count was not overwritten"
        return got

    def refused(self, k, **kw):
        """The call returns an error and leaves count and every sentinel as they were."""
        from ssv_amd import _lib
        rc = self.raw(k, **kw)
        assert rc != 0 and b"ssv_knn_label_agreement" in _lib.load().ssv_last_error(), (rc, kw)
        assert int(self.cbuf[0].item()) == COUNT_PATTERN, "a refused call wrote count"
        self.check_untouched("refused call")


def run_case(c):
    """{labelling: count} of the case through the guarded ABI call, with the second call and the ops call compared on the way."""
    from ssv_amd import ops
    z = case_features(c)
    g = Guarded(z, c.arith)
    counts = {}
    for name, lab in ko.labelings(c.n):
        g.set_labels(lab)
        counts[name] = g.count(c.k)
    assert g.count(c.k) == counts[name], "a second identical call returned another count"
    with ops.arithmetic(c.arith):
        via_ops = ops.knn_label_agreement(torch.tensor(z).cuda(), torch.tensor(np.asarray(lab, np.int32)).cuda(), c.k)
    assert via_ops == counts[name], ("ops.knn_label_agreement", via_ops, counts[name])
    return counts


def _parts(c):
    if not c.labels[0].startswith("fused."):
        return None
    return choose_parts(c.n, torch.cuda.get_device_properties(0).multi_processor_count)[0]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_KNN_AGREE_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "device": torch.cuda.get_device_properties(0).name,
                       "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


# ====================================================================================================================== exact cases
@pytest.mark.parametrize("case", ROUTE_CASES + CONTENT_CASES, ids=lambda c: c.id)
def test_counts_are_exact_on_integer_features(case):
    c = case
    idx = neighbour_lists(c.family, c.n, c.d, c.k, c.seed)
    want = {name: ko.count(idx, lab) for name, lab in ko.labelings(c.n)}
    got = run_case(c)
    REPORT[c.id] = {"route": c.labels[0], "labels": list(c.labels), "parts": _parts(c), "counts": got, "expected": want}
    wrong = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    print(f"{c.id}: parts {_parts(c)}, equal-labelling count {got['equal']} of {c.n * c.k}, wrong labellings {len(wrong)}")
    assert not wrong, wrong
    if c.family == "nan":                                   # the NaN row is nobody's neighbour and has none; every other list is full
        assert want["equal"] == (c.n - 1) * c.k and not (idx == c.n - 1).any() and (idx[c.n - 1] == -1).all()
    else:
        assert want["equal"] == c.n * c.k
    if "fallback.f32" in c.labels:                          # bit-identical to the run that asks for f32
        assert run_case(c._replace(arith="f32")) == got


# ====================================================================================================================== fp32 features
@pytest.mark.parametrize("case", FP32_CASES, ids=lambda c: c.id)
def test_counts_stay_inside_the_window_on_fp32_features(case):
    c = case
    z = case_features(c)
    m = case_margins(c.family, c.n, c.d, c.k, c.seed)
    got = run_case(c)
    windows = {name: ko.window(z, lab, c.k, m)[:2] for name, lab in ko.labelings(c.n)}
    REPORT[c.id] = {"route": c.labels[0], "labels": list(c.labels), "parts": _parts(c), "counts": got, "windows": {k: list(v) for k, v in windows.items()},
                    "excused_share": m.excused_share}
    outside = {name: (got[name], windows[name]) for name in windows if not windows[name][0] <= got[name] <= windows[name][1]}
    print(f"{c.id}: parts {_parts(c)}, excused {m.excused_share:.2%}, widest window {max(h - l for l, h in windows.values())}, outside {len(outside)}")
    assert not outside, outside
    assert got["equal"] == c.n * c.k                        # (all distinct: a query counts itself wherever the dropped hit is another row - the window says how often)


# ====================================================================================================================== the table on this device
def test_fused_cases_reach_one_part_and_several_parts_on_this_device():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    parts = {c.id: choose_parts(c.n, cus)[0] for c in CASES if c.labels[0].startswith("fused.")}
    print(f"{cus} compute units: parts per fused case {sorted(set(parts.values()))}")
    assert 1 in parts.values() and max(parts.values()) > 1, parts


# ====================================================================================================================== refusals
def test_refusals_leave_count_and_the_sentinels_untouched():
    z = features("ints", 300, 32, 0)
    for arith in ARITHMETICS:
        g = Guarded(z, arith)
        g.set_labels(ko.labelings(300)[3][1])
        want = g.count(20)
        g.refused(300)                                      # k >= n
        g.refused(299, n=299)                               # k == n with a smaller n
        g.refused(64)                                       # k > 63
        g.refused(20, d=30)                                 # d % 4 != 0
        g.refused(20, ws_bytes=g.ws_bytes - 1)              # a workspace one byte short
        g.refused(20, z_off=4)                              # a misaligned z
        g.refused(0)
        assert g.count(20) == want                          # and the next good call is unaffected
