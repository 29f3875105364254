"""GPU: every launch form of csrc/kmeans.hip - ssv_kmeans_assign, ssv_kmeans_update and ssv_cluster_votes straight through the C ABI, so that prep, prep_ready,
the workspace and the guards are the test's - against the fp64 oracle of tests/kmeans_oracle.py, in BOTH arithmetics (bf16x3: kmeans_fused_k<KT>; f32: the GEMM
through the workspace and kmeans_rowarg_k).  The inputs are kmeans_oracle.form_case(i): seeded blobs and three centroid sets (initial rows, one and two fp64
updates rounded to fp32); tests/test_kmeans_cpu.py proves in fp64 alone that they are no near-tie inputs and that every centroid of every set wins a row, and
keeps this table honest.

Held, for every case and centroid set:
  1. the assignment contract of tests/test_gpu_kmeans.py (_check_assignment, imported): exact fp64 labels outside the excused rows, excused share <= 1 %,
     tau_i on dist, sum tau_i on the objective, counts == bincount(labels);
  2. rule (a) of tests/test_gpu_loss_kernels.py (tests/forms_report.py) on dist and on the objective, family kmeans.dist: tau is 2^-14 relative, a lost third
     bf16 piece would pass it.  ref64 / ref32 = kmeans_oracle.dist_at at the fp64 label in float64 / float32 (the objective: its sum).  Where ref64 is
     identically zero the relative errors do not exist; that is the case for form.21 alone (n = k = 1: the row is its own centroid in every set - ZERO_REFERENCE,
     proved in tests/test_kmeans_cpu.py), which is held by 1. only;
  3. labels, dist, counts, objective, prep and the workspace are views with 1024 guard elements behind them (NaN, or a sentinel for the integer buffers), sized
     by ssv_kmeans_prep_bytes / ssv_kmeans_workspace_bytes exactly; counts and the workspace hold garbage before the call; afterwards no output element keeps its
     prefill (of prep: every word but the alignment gap between 1/2 |c|^2 and the planes), every guard is untouched, x and the centroids are bit-identical;
  4. after ssv_kmeans_update(..., prep) the bytes of prep are those an assignment with prep_ready = 0 writes for the updated centroids, and an assignment with
     prep_ready = 1 on it returns the bits of the one with prep_ready = 0;
  5. the update within kmeans_oracle.update_bound on the GPU's own labels, empty clusters bit-identical;
  7. a second call on equal inputs - with the OTHER workspace prefill - gives equal bits.

Branch labels (label, entry point, what the case reaches; form.NN rows: the case (n, d, k, spread) first):

  form.00            ssv_kmeans_assign   (257, 64, 1, 1.0)      KT 1, k = 1; d = 64: one chunk, reloaded by the prefetch; three row blocks, the last holding one row
  form.01            ssv_kmeans_assign   (300, 32, 31, 1.0)     KT 1, padded tile
  form.02            ssv_kmeans_assign   (300, 32, 32, 1.0)     KT 1, full tile
  form.03            ssv_kmeans_assign   (400, 64, 64, 2.0)     KT 2, full
  form.04            ssv_kmeans_assign   (500, 68, 70, 2.0)     KT 4 with T = 3 (one repeated tile); d = 68: the second chunk holds 4 real columns
  form.05            ssv_kmeans_assign   (700, 60, 130, 2.0)    KT 8 with T = 5; d % 16 != 0
  form.06            ssv_kmeans_assign   (900, 128, 200, 2.0)   KT 8 with T = 7, padded
  form.07            ssv_kmeans_assign   (1500, 128, 250, 2.0)  PCL's k = 250: T = 8, padded
  form.08            ssv_kmeans_assign   (1200, 16, 257, 1.0)   two passes, the second with ONE live tile holding ONE real centroid
  form.09            ssv_kmeans_assign   (1500, 48, 300, 2.0)   two passes, the second with 2 of 8 tiles
  form.10            ssv_kmeans_assign   (2000, 128, 500, 3.0)  PCL's k = 500
  form.11            ssv_kmeans_assign   (3000, 128, 1000, 3.0) PCL's k = 1000
  form.12            ssv_kmeans_assign   (1100, 16, 1024, 1.0)  k <= HIST: the LDS histogram at its largest
  form.13            ssv_kmeans_assign   (1100, 16, 1025, 1.0)  k > HIST: the global counters; k % 4 != 0
  form.14            ssv_kmeans_assign   (130, 8192, 3, 4.0)    d = SSV_KMEANS_MAX_D: 128 chunks
  form.15            ssv_kmeans_assign   (200, 4096, 40, 4.0)   d > 2048 with two tiles
  form.16            ssv_kmeans_assign   (129, 4, 5, 1.0)       d = 4: one float4 per row, 15 of 16 slab columns zero; n = 128 + 1
  form.17            ssv_kmeans_assign   (127, 36, 9, 1.0)      n one short of a row block
  form.18            ssv_kmeans_assign   (128, 36, 9, 1.0)      n exactly one row block
  form.19            ssv_kmeans_assign   (4097, 16, 7, 1.0)     unfused route: a second row chunk of ONE row; k % 4 != 0 (scalar GEMM epilogue, unaligned rows of S)
  form.20            ssv_kmeans_update   (8195, 16, 4096, 1.0)  three one-hot chunks (4096 rows each at kp = 4096), the last of 3 rows, accumulate on chunks 2 and 3
  form.21            ssv_kmeans_assign   (1, 4, 1, 1.0)         n = k = 1
  buffers.guarded    ssv_kmeans_assign   check 3 on every case
  det.assign         ssv_kmeans_assign   check 7: the second assignment, workspace prefilled with the other pattern
  det.update         ssv_kmeans_update   check 7: the second update
  prep.ready         ssv_kmeans_assign   check 4: prep_ready = 1 on what ssv_kmeans_update left
  prep.bytes         ssv_kmeans_update   check 4: the bytes of prep
  update.own_labels  ssv_kmeans_update   check 5 on every case
  update.bad_label   ssv_kmeans_update   form.13 (kp = 1028 > k): labels -1, k, k + 2 and 2^31 - 1 contribute to no centroid, nothing behind centroids[k] is written
  update.zero_count  ssv_kmeans_update   form.03: counts[j] = 0 for a cluster with members and a negative count for another: both centroids bit-unchanged
  dup.half_wave      ssv_kmeans_assign   form.10 with centroid 5 a copy of 2: the same tile, the other half-wave
  dup.tile           ssv_kmeans_assign   40 a copy of 3: another tile of the same pass
  dup.pass           ssv_kmeans_assign   300 a copy of 7: another pass
  dup.pad_tile       ssv_kmeans_assign   499 a copy of 10: the padded last tile
  dup.unfused_trip   ssv_kmeans_assign   75 a copy of 11: another trip of the unfused route's j += 64 loop
  votes.table        ssv_cluster_votes   the table against a histogram: votes zeroed by the call, flag 0; n = 1, one cell, several blocks
  votes.flag         ssv_cluster_votes   labels -1, pred_k and 2^31 - 1: not counted, flag raised

FACTOR / FLOOR: see below and profiles/kmeans_pirl_forms_report.json.
"""
import functools
import re

import numpy as np
import pytest
import torch

import forms_report as fr
import kmeans_oracle as ko
from test_gpu_kmeans import _check_assignment

pytestmark = pytest.mark.gpu
ARITHMETICS = ("bf16x3", "f32")
MAX_D = 8192
ZERO_REFERENCE = (21,)                                                   # form cases whose distances are identically zero in fp64: rule (a) has no scale there
# family kmeans.dist, by the rule of tests/forms_report.py from the MI355X run committed as profiles/kmeans_pirl_forms_report.json: the worst ratio is 1.75
# (m of dist, form.14 in bf16x3).  Before the kernels summed |x - c|^2 directly the same run gave 34 (m of dist, form.15 in bf16x3: a chain of d / 2 additions
# per lane for |x|^2), 13.8 on the f32 route there, and 110 on the objective of form.12 (one-sided noise on the rows that are their own centroid)
FACTOR = 2.0
FLOOR = 2 * fr.U                                                         # the final rounding of an fp32 result, and of the partial sum it is folded from
FAMILY = fr.Family("kmeans.dist", FACTOR, FLOOR)
DUPLICATES = ((2, 5, "dup.half_wave"), (3, 40, "dup.tile"), (7, 300, "dup.pass"), (10, 499, "dup.pad_tile"), (11, 75, "dup.unfused_trip"))

_FORMS = " ".join(f"form.{i:02d}" for i in range(len(ko.FORM_CASES)))
TARGETS = {
    "test_assignment_forms_against_fp64": _FORMS + " buffers.guarded det.assign",
    "test_update_and_prep_ready_on_every_form": _FORMS + " update.own_labels prep.ready prep.bytes det.update",
    "test_update_leaves_out_labels_outside_the_range": "update.bad_label",
    "test_update_keeps_centroids_whose_count_is_not_positive": "update.zero_count",
    "test_duplicates_never_win_against_their_first_copy": " ".join(d[2] for d in DUPLICATES),
    "test_cluster_votes_table_and_flag": "votes.table votes.flag",
}


def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(ssv_\w+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def documented_form_cases():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  form\.(\d+)\s+ssv_\w+\s+\((\d+), (\d+), (\d+), ([0-9.]+)\)", line)
        if m:
            out[int(m.group(1))] = (int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)))
    return out


errors = fr.errors


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from ssv_amd import _lib
    yield _lib.load()
    fr.write([FAMILY])


def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


@functools.lru_cache(maxsize=None)
def _want_labels(index, which):
    x, sets = ko.form_case(index)
    return ko.assign(x, sets[which])[0]


def _workspace(lib, b, n, d, k, arith, fill):
    nbytes = lib.ssv_kmeans_workspace_bytes(n, d, k, _code(arith))
    assert nbytes > 0 and nbytes % 4 == 0
    return b.out("ws", nbytes // 4, torch.int32, fill), nbytes


def _prep(lib, b, d, k, name="prep"):
    nbytes = lib.ssv_kmeans_prep_bytes(d, k)
    assert nbytes > 0 and nbytes % 4 == 0
    return b.out(name, nbytes // 4, torch.int32, -1)                    # 0xFFFFFFFF: neither a finite float nor two bf16 pieces of one


def _assign(lib, b, xd, cd, arith, prep=None, ready=0, ws_fill=fr.NAN_BITS, tag=""):
    """One guarded ssv_kmeans_assign; returns (labels, dist, counts, objective, prep)."""
    from ssv_amd import _lib
    (n, d), k = xd.shape, cd.shape[0]
    if prep is None:
        prep = _prep(lib, b, d, k, "prep" + tag)
    labels = b.out("labels" + tag, n, torch.int32, -5)
    dist = b.out("dist" + tag, n, torch.float32, float("nan"))
    counts = b.out("counts" + tag, k, torch.int32, fr.GARBAGE)
    objective = b.out("objective" + tag, 1, torch.float32, float("nan"))
    ws, nbytes = _workspace(lib, b, n, d, k, arith, ws_fill)
    P = _lib.ptr
    _lib.call("ssv_kmeans_assign", n, d, k, P(xd), P(cd), P(prep), ready, P(labels), P(dist), P(counts), P(objective), _code(arith), P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert bool((labels != -5).all()) and not bool(torch.isnan(dist).any()) and not bool(torch.isnan(objective).any()), "an output element kept its prefill"
    assert bool(((counts >= 0) & (counts <= n)).all()) and int(counts.sum()) == n, "counts were not zeroed by the call"
    kpad = 32 * ((k + 31) // 32)                                         # geo() of csrc/kmeans.hip: hc [kpad] floats, then the planes from the next multiple of 256 bytes
    gap = torch.zeros(prep.numel(), dtype=torch.bool, device="cuda")
    gap[kpad:(kpad * 4 + 255) // 256 * 64] = True
    assert bool(((prep != -1) | gap).all()), f"{int(((prep == -1) & ~gap).sum())} words of prep were never written"
    return labels, dist, counts, objective, prep


def _update(lib, b, xd, labels, counts, cd, arith, prep, ws_fill=fr.GARBAGE):
    from ssv_amd import _lib
    (n, d), k = xd.shape, cd.shape[0]
    ws, nbytes = _workspace(lib, b, n, d, k, arith, ws_fill)
    P = _lib.ptr
    _lib.call("ssv_kmeans_update", n, d, k, P(xd), P(labels), P(counts), P(cd), P(prep), _code(arith), P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()


def _same(a, b_, what):
    for name, u, v in zip(("labels", "dist", "counts", "objective"), a, b_):
        assert torch.equal(fr.bits(u), fr.bits(v)), f"{what}: {name} differ"


@pytest.mark.parametrize("arith", ARITHMETICS)
@pytest.mark.parametrize("index", range(len(ko.FORM_CASES)))
def test_assignment_forms_against_fp64(lib, index, arith):
    x, sets = ko.form_case(index)
    fails = []
    for which, c in enumerate(sets):
        what = f"form.{index:02d} {ko.FORM_CASES[index]} set {which} [{arith}]"
        b = fr.Buffers()
        xd, cd = b.up("x", x), b.up("centroids", c)
        first = _assign(lib, b, xd, cd, arith, ws_fill=fr.NAN_BITS)
        _check_assignment(x, c, *first[:4])
        again = _assign(lib, b, xd, cd, arith, ws_fill=fr.GARBAGE, tag=" (second call)")
        _same(first, again, what)
        assert torch.equal(first[4], again[4]), f"{what}: prep differs between two calls"
        b.verify(what)
        want = _want_labels(index, which)
        r64, r32 = ko.dist_at(x, c, want, np.float64), ko.dist_at(x, c, want, np.float32)
        if index in ZERO_REFERENCE:
            assert not np.abs(r64).max() > 0
            continue
        assert np.abs(r64).max() > 0
        # an excused row may carry another label (check 1.): its distance is then the one to THAT centroid, up to tau_i from the best - a property of the
        # data, not of the arithmetic rule (a) is about.  Such rows are left out of dist, and the objective's reference takes their distance at the label given
        got = first[0].cpu().numpy().astype(np.int64)
        keep = got == want
        assert keep.mean() >= 1.0 - ko.MAX_EXCUSED
        FAMILY.hold(what, "dist", first[1].cpu().numpy()[keep], r64[keep], r32[keep], fails)
        if not keep.all():
            r64, r32 = ko.dist_at(x, c, got, np.float64), ko.dist_at(x, c, got, np.float32)
        FAMILY.hold(what, "objective", first[3].cpu().numpy(), r64.sum(), r32.sum(dtype=np.float32), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("arith", ARITHMETICS)
@pytest.mark.parametrize("index", range(len(ko.FORM_CASES)))
def test_update_and_prep_ready_on_every_form(lib, index, arith):
    x, sets = ko.form_case(index)
    n, d, k, _ = ko.FORM_CASES[index]
    for which, c in enumerate(sets):
        what = f"form.{index:02d} {ko.FORM_CASES[index]} set {which} [{arith}]"
        b = fr.Buffers()
        xd, c0 = b.up("x", x), b.up("centroids before", c)
        labels, _, counts, _, _ = _assign(lib, b, xd, c0, arith)
        b.inputs += [("labels", labels, labels.clone()), ("counts", counts, counts.clone())]
        cd = b.out("centroids", k * d, torch.float32, c0.reshape(-1)).view(k, d)
        prep_u = _prep(lib, b, d, k, "prep (update)")
        _update(lib, b, xd, labels, counts, cd, arith, prep_u)
        lab = labels.cpu().numpy().astype(np.int64)
        want, bound = ko.update(x, lab, c), ko.update_bound(x, lab, k)
        err = np.abs(cd.cpu().numpy().astype(np.float64) - want)
        print(f"{what}: max update err / bound {float((err / np.maximum(bound, 1e-300))[bound > 0].max()):.3e}")
        assert (err <= bound).all(), (what, float((err - bound).max()))
        empty = torch.as_tensor(np.bincount(lab, minlength=k) == 0)
        assert torch.equal(fr.bits(cd).cpu()[empty], fr.bits(c0).cpu()[empty]), f"{what}: an empty cluster's centroid moved"
        # the second update, from the same centroids, with the other workspace prefill
        cd2 = b.out("centroids (second call)", k * d, torch.float32, c0.reshape(-1)).view(k, d)
        prep_2 = _prep(lib, b, d, k, "prep (second update)")
        _update(lib, b, xd, labels, counts, cd2, arith, prep_2, ws_fill=fr.NAN_BITS)
        assert torch.equal(fr.bits(cd), fr.bits(cd2)) and torch.equal(prep_u, prep_2), f"{what}: two updates differ"
        # prep as the update left it against a fresh one, then prep_ready = 1 against 0
        b.inputs.append(("updated centroids", cd, cd.clone()))
        fresh = _assign(lib, b, xd, cd, arith, tag=" (fresh)")
        assert torch.equal(prep_u, fresh[4]), f"{what}: {int((prep_u != fresh[4]).sum())} words of prep differ from what an assignment makes"
        b.inputs.append(("prep", prep_u, prep_u.clone()))
        ready = _assign(lib, b, xd, cd, arith, prep=prep_u, ready=1, ws_fill=fr.GARBAGE, tag=" (prep_ready)")
        _same(fresh, ready, what + " prep_ready")
        b.verify(what)


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_update_leaves_out_labels_outside_the_range(lib, arith):
    index = 13
    x, sets = ko.form_case(index)
    n, d, k, _ = ko.FORM_CASES[index]
    assert (k + 3) // 4 * 4 == 1028 and k == 1025
    lab = _want_labels(index, 0).copy()
    rows = ko.init_rows(77, n, 8)
    lab[rows] = [-1, k, k + 2, 2 ** 31 - 1, -1, k, k + 2, 2 ** 31 - 1]
    valid = np.ones(n, bool)
    valid[rows] = False
    counts = np.bincount(lab[valid], minlength=k)
    b = fr.Buffers()
    xd, labels, cnt = b.up("x", x), b.up("labels", lab, torch.int32), b.up("counts", counts, torch.int32)
    cd = b.out("centroids", k * d, torch.float32, torch.as_tensor(sets[0]).reshape(-1)).view(k, d)
    _update(lib, b, xd, labels, cnt, cd, arith, _prep(lib, b, d, k))
    want, bound = ko.update(x[valid], lab[valid], sets[0]), ko.update_bound(x[valid], lab[valid], k)
    err = np.abs(cd.cpu().numpy().astype(np.float64) - want)
    assert (err <= bound).all(), float((err - bound).max())
    b.verify(f"form.13 with labels outside [0, k) [{arith}]")


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_update_keeps_centroids_whose_count_is_not_positive(lib, arith):
    index = 3
    x, sets = ko.form_case(index)
    n, d, k, _ = ko.FORM_CASES[index]
    lab = _want_labels(index, 0)
    counts = np.bincount(lab, minlength=k)
    assert counts[4] > 0 and counts[37] > 0                             # both have members
    given = counts.copy()
    given[4], given[37] = 0, -3
    b = fr.Buffers()
    xd, labels, cnt = b.up("x", x), b.up("labels", lab, torch.int32), b.up("counts", given, torch.int32)
    before = torch.as_tensor(sets[0]).cuda()
    cd = b.out("centroids", k * d, torch.float32, before.reshape(-1)).view(k, d)
    _update(lib, b, xd, labels, cnt, cd, arith, _prep(lib, b, d, k))
    assert torch.equal(fr.bits(cd)[[4, 37]], fr.bits(before)[[4, 37]])
    want, bound = ko.update(x, lab, sets[0]), ko.update_bound(x, lab, k)
    err = np.abs(cd.cpu().numpy().astype(np.float64) - want)
    others = np.ones(k, bool)
    others[[4, 37]] = False
    assert (err[others] <= bound[others]).all() and not torch.equal(fr.bits(cd)[5], fr.bits(before)[5])
    b.verify(f"form.03 with counts <= 0 [{arith}]")


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_duplicates_never_win_against_their_first_copy(lib, arith):
    index = 10
    x, sets = ko.form_case(index)
    los, his = [p[0] for p in DUPLICATES], [p[1] for p in DUPLICATES]
    for which in (0, 1):
        c = sets[which].copy()
        c[his] = c[los]                                                  # bit-identical rows
        b = fr.Buffers()
        labels, _, counts, _, _ = _assign(lib, b, b.up("x", x), b.up("centroids", c), arith)
        labels, counts = labels.cpu().numpy().astype(np.int64), counts.cpu().numpy()
        assert not np.isin(labels, his).any() and (counts[his] == 0).all(), (which, [h for h in his if (labels == h).any()])
        dm = ko.sqdist(x, c)
        dm[:, his] = np.inf
        want = dm.argmin(1)
        two = np.partition(dm, 1, axis=1)[:, :2]
        held = (two[:, 1] - two[:, 0] >= ko.margins(x, c)[2]) & np.isin(want, los)
        for lo in los:
            assert (held & (want == lo)).any(), (which, lo)               # the case measures something for every pair
        assert np.array_equal(labels[held], want[held]), (which, np.nonzero(held & (labels != want))[0][:10])
        b.verify(f"form.10 set {which} with duplicates [{arith}]")


def test_cluster_votes_table_and_flag(lib):
    from ssv_amd import _lib
    P = _lib.ptr
    rng = np.random.default_rng(11)

    def run(pred, tgt, pk, tk):
        b = fr.Buffers()
        pd, td = b.up("pred", pred, torch.int32), b.up("targets", tgt, torch.int32)
        votes = b.out("votes", pk * tk, torch.int64, fr.GARBAGE)
        flag = b.out("flag", 1, torch.int32, fr.GARBAGE)
        _lib.call("ssv_cluster_votes", len(pred), P(pd), P(td), pk, tk, P(votes), P(flag), _lib.stream())
        b.verify(f"votes {len(pred)} x {pk} x {tk}")
        return votes.cpu().numpy().reshape(pk, tk), int(flag)

    for n, pk, tk in ((5000, 7, 12), (1, 3, 2), (300, 1, 1), (257, 33, 5)):
        pred, tgt = rng.integers(0, pk, n), rng.integers(0, tk, n)
        votes, flag = run(pred, tgt, pk, tk)
        want = np.histogram2d(pred, tgt, bins=(np.arange(pk + 1), np.arange(tk + 1)))[0].astype(np.int64)
        assert flag == 0 and np.array_equal(votes, want)
    n, pk, tk = 600, 4, 6
    pred, tgt = rng.integers(0, pk, n), rng.integers(0, tk, n)
    pred[17], tgt[3], pred[300], tgt[599] = pk, -1, 2 ** 31 - 1, tk
    ok = np.ones(n, bool)
    ok[[17, 3, 300, 599]] = False
    votes, flag = run(pred, tgt, pk, tk)
    want = np.histogram2d(pred[ok], tgt[ok], bins=(np.arange(pk + 1), np.arange(tk + 1)))[0].astype(np.int64)
    assert flag != 0 and np.array_equal(votes, want) and votes.sum() == n - 4
