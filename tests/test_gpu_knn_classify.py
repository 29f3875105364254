"""GPU: the weighted kNN classifier (csrc/knnclassify.hip through ops / utils.eval_utils, the trainer and the command line) against the fp64 oracle of
tests/knn_classify_oracle.py.

Search.  Integer features ({-2 .. 2}, d 64): every product is exact in both arithmetics, so idx and sim ARE the oracle's, tie rule included, whatever the
partition.  fp32 features (unit-length blobs): with tau_i = 2^-14 |q_i| max_j |b_j| (the k-means tolerance of DESIGN 7.6 applied to the product term alone),
(i) every returned sim is within tau_i of the fp64 similarity of the returned index, (ii) sim is non-increasing and equal neighbours have ascending indices,
(iii) every bank row whose fp64 similarity exceeds the fp64 k-th best by more than 2 tau_i is present and no returned row lies more than 2 tau_i below it,
(iv) no duplicate and no out-of-range index.
Vote.  Fed with the ORACLE's neighbour lists, so it does not depend on the search.  scores under rules (a) and (d) of tests/test_gpu_loss_kernels.py:
e(got) <= FACTOR e(ref32) + FLOOR and the same for m, with ref64 = the oracle, ref32 = the same lines in torch fp32 on the CPU (summed in rank order),
FLOOR = 2 * 2^-24 (the final rounding of an fp32 result; at most 16 * 2^-24 is allowed) and FACTOR the worst max(0, e(got) - FLOOR) / e(ref32) (and the same
for m) measured on an MI355X (profiles/knn_classify_report.json, written by this file under SSV_KNN_CLASSIFY_REPORT=<path>), rounded up to the next power of
two and never above 8.  Measured: 0 for seven of the eight cases (e and m of the kernel at or below FLOOR above ref32's), 0.25 for m at k 1024, C 1000, T 0.07
(1.60e-7, the bits of ref32 itself) - so FACTOR is 1.  Outputs are views into NaN-prefilled buffers with 1024 floats of guard, inputs are bit-identical afterwards.
pred equals the fp64 prediction wherever the fp64 relative margin between the two best class scores exceeds MU = 2^-13 (<= 1024 positive fp32 additions,
<= 2^-14, and the rounding of an exponent argument of at most 2 / 0.07, ~ 2^-18, for each of the two scores); at most 1 % of the queries may fall under it
(tests/test_knn_classify_cpu.py: none does), and every row of pred is the stable arg-sort of the kernel's OWN scores.
End to end.  eval_utils.knn_classify == ops.knn_search + ops.knn_vote bit for bit; integer family: the oracle's predictions; blobs: each prediction equals the
fp64 vote over the RETURNED neighbour list with fp64 similarities unless the query's fp64 relative margin is below 2 tau_i / T + MU (at most 1 % of them)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import knn_classify_oracle as kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITHMETICS = ("bf16x3", "f32")
U = 2.0 ** -24
GUARD = 1024
FACTOR = 1.0                                              # measured worst ratio 0.25 (see above; profiles/knn_classify_report.json), rounded up to a power of two
FLOOR = 2 * U
REPORT = {}
# (k, C, topn, blob shape the neighbour lists come from)
VOTE_CASES = ((1, 1, 1, 0), (20, 10, 1, 0), (200, 100, 1, 1), (1024, 1000, 5, 1))
VOTE_TEMPERATURES = (0.07, 1.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_KNN_CLASSIFY_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _np(sim, idx):
    return sim.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)


# ====================================================================================================================== search, exact
@pytest.mark.parametrize("arith", ARITHMETICS)
def test_search_is_exact_on_integer_features(arith):
    from ssv_amd import ops
    bank, _, queries, _ = kc.integers()
    n = bank.shape[0]
    bd, qd = _dev(bank), _dev(queries)
    with ops.arithmetic(arith):
        for k in kc.KS + (n,):
            want_sim, want_idx = kc.search(queries, bank, k)
            sim, idx = ops.knn_search(qd, bd, k)
            got_sim, got_idx = _np(sim, idx)
            assert sim.shape == (queries.shape[0], k) and idx.dtype == torch.int32
            assert np.array_equal(got_idx, want_idx), (k, np.argwhere(got_idx != want_idx)[:5])
            assert np.array_equal(got_sim, want_sim), k
            # four parts (the last one 232 columns wide) and three chunks (the last one 44 rows): the same bits
            sim2, idx2 = ops.knn_search(qd, bd, k, chunk_rows=128, part_cols=256)
            assert torch.equal(idx2, idx) and torch.equal(_bits(sim2), _bits(sim)), k
        sim3, idx3 = ops.knn_search(qd, bd, 200, part_cols=128)          # every part is narrower than k
        want_sim, want_idx = kc.search(queries, bank, 200)
        assert np.array_equal(_np(sim3, idx3)[1], want_idx) and np.array_equal(_np(sim3, idx3)[0], want_sim)
        again = ops.knn_search(qd, bd, 200, part_cols=128)
        assert torch.equal(again[1], idx3) and torch.equal(_bits(again[0]), _bits(sim3))


# ====================================================================================================================== search, fp32 features
def _check_search(queries, bank, k, sim, idx):
    """(i) - (iv) of the module docstring."""
    got_sim, got_idx = _np(sim, idx)
    m, n = queries.shape[0], bank.shape[0]
    s = kc.similarities(queries, bank)
    tau = kc.tau(queries, bank)[:, None]
    assert got_idx.min() >= 0 and got_idx.max() < n                                                     # (iv)
    srt = np.sort(got_idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    s_ret = np.take_along_axis(s, got_idx, axis=1)
    err = np.abs(got_sim - s_ret)
    print(f"m={m} n={n} d={queries.shape[1]} k={k}: max |sim err| / tau {float((err / tau).max()):.3e}")
    assert (err <= tau).all(), float((err / tau).max())                                                 # (i)
    d = np.diff(got_sim, axis=1)
    assert (d <= 0).all() and (np.diff(got_idx, axis=1)[d == 0] > 0).all()                              # (ii)
    kth = -np.partition(-s, k - 1, axis=1)[:, k - 1:k]                                                  # (iii)
    present = np.zeros((m, n), bool)
    np.put_along_axis(present, got_idx, True, axis=1)
    assert present[s > kth + 2 * tau].all()
    assert (s_ret >= kth - 2 * tau).all()


@pytest.mark.parametrize("index,arith", ((0, "bf16x3"), (0, "f32"), (1, "bf16x3")))
def test_search_on_fp32_features(index, arith):
    """d = 36 has no bf16-piece kernel: it takes the fp32-MFMA route whatever is asked for."""
    from ssv_amd import ops
    bank, _, queries, _ = kc.blobs(index)
    n = bank.shape[0]
    bd, qd = _dev(bank), _dev(queries)
    with ops.arithmetic(arith):
        for k in kc.KS + ((n,) if n <= 1024 else (1024,)):
            _check_search(queries, bank, k, *ops.knn_search(qd, bd, k))
        _check_search(queries, bank, 200, *ops.knn_search(qd, bd, 200, chunk_rows=100, part_cols=384))


# ====================================================================================================================== edges of the selection
@pytest.mark.parametrize("arith", ARITHMETICS)
def test_selection_edges(arith):
    from ssv_amd import ops
    bank, _, queries, _ = kc.integers()
    n = bank.shape[0]
    with ops.arithmetic(arith):
        # an all-zero query: every score ties, the lowest indices win
        q = queries[:3].copy()
        q[1] = 0.0
        for k in (1, 20, 200, n):
            idx = ops.knn_search(_dev(q), _dev(bank), k)[1].cpu().numpy()
            assert np.array_equal(idx[1], np.arange(k)), k
        # the negative of a bank row against a bank shifted to {1 .. 5}: every score of the row is negative
        shifted = bank + 3.0
        q = np.stack([-shifted[7], queries[0]])
        for k in (1, 20, n):
            want_sim, want_idx = kc.search(q, shifted, k)
            assert (want_sim[0] < 0).all()
            got_sim, got_idx = _np(*ops.knn_search(_dev(q), _dev(shifted), k))
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got_sim, want_sim), k
        # one bank row holding a NaN: last with k = n, absent with k = 20
        nanbank = bank.copy()
        nanbank[13, 5] = np.nan
        want_sim, want_idx = kc.search(queries, nanbank, n)
        got_sim, got_idx = _np(*ops.knn_search(_dev(queries), _dev(nanbank), n))
        assert (got_idx[:, -1] == 13).all() and np.isnan(got_sim[:, -1]).all() and not np.isnan(got_sim[:, :-1]).any()
        assert np.array_equal(got_idx, want_idx) and np.array_equal(got_sim[:, :-1], want_sim[:, :-1])
        got_sim, got_idx = _np(*ops.knn_search(_dev(queries), _dev(nanbank), 20, part_cols=256))
        assert not (got_idx == 13).any() and np.array_equal(got_idx, kc.search(queries, nanbank, 20)[1])
        # n = 1003 and m = 1: the row stride of S is not a multiple of 4
        g = torch.Generator().manual_seed(77)
        odd = torch.randint(-2, 3, (1003, 64), generator=g).float().numpy()
        for k in (1, 200, 1003):
            want_sim, want_idx = kc.search(queries[:1], odd, k)
            got_sim, got_idx = _np(*ops.knn_search(_dev(queries[:1]), _dev(odd), k))
            assert np.array_equal(got_idx, want_idx) and np.array_equal(got_sim, want_sim), k
    # duplicate bank rows 2 and 5 (fp32 features): row 5 never ranks ahead of row 2
    fbank, _, fq, _ = kc.blobs(0)
    fbank = fbank.copy()
    fbank[5] = fbank[2]
    with ops.arithmetic(arith):
        for k, pc in ((20, 0), (200, 0), (fbank.shape[0], 0), (200, 256)):
            idx = ops.knn_search(_dev(fq), _dev(fbank), k, part_cols=pc)[1].cpu().numpy()
            has2, has5 = (idx == 2).any(1), (idx == 5).any(1)
            assert not (has5 & ~has2).any() and has5.any()
            both = has2 & has5
            assert ((idx[both] == 2).argmax(1) + 1 == (idx[both] == 5).argmax(1)).all()          # equal scores: adjacent, the lower index first


# ====================================================================================================================== vote
def vote_inputs(case):
    """(sim [m, k] fp32, idx [m, k] int32, bank labels [n] int64, C): the oracle's neighbour lists of a blob shape, similarities rounded to fp32 (what the kernel is given)."""
    k, c, _, index = case
    bank, yb, queries, _ = kc.blobs(index)
    sim, idx = kc.search(queries, bank, k)
    if c == 1:
        labels = np.zeros(bank.shape[0], np.int64)
    elif c == kc.BLOB_SHAPES[index][3]:
        labels = yb.astype(np.int64)
    else:
        labels = torch.randint(0, c, (bank.shape[0],), generator=torch.Generator().manual_seed(31 + c)).numpy()
    return sim.astype(np.float32), idx.astype(np.int32), labels, c


def _err(x, ref64):
    d = np.asarray(x, np.float64) - ref64
    return float(np.linalg.norm(d) / max(np.linalg.norm(ref64), 1e-300)), float(np.abs(d).max() / max(np.abs(ref64).max(), 1e-300))


def _ratio(got, ref, floor):
    if got <= floor:
        return 0.0
    return (got - floor) / ref if ref > 0 else float("inf")


def _vote_abi(sim_d, idx_d, lab_d, c, topn, inv_temp, want_scores=True):
    """ssv_knn_vote straight through the C ABI into guarded buffers: (pred, scores, flag) after the checks of rule (d)."""
    from ssv_amd import _lib
    m, k = sim_d.shape
    keep = [t.clone() for t in (sim_d, idx_d, lab_d)]
    sbuf = torch.full((m * c + GUARD,), float("nan"), device="cuda")
    pbuf = torch.full((m * topn + 64,), -77, dtype=torch.int32, device="cuda")
    fbuf = torch.full((1 + 64,), -77, dtype=torch.int32, device="cuda")
    _lib.call("ssv_knn_vote", m, k, lab_d.numel(), c, topn, _lib.ptr(sim_d), _lib.ptr(idx_d), _lib.ptr(lab_d), inv_temp, _lib.ptr(pbuf),
              _lib.ptr(sbuf) if want_scores else 0, _lib.ptr(fbuf), _lib.stream())
    torch.cuda.synchronize()
    for t, was in zip((sim_d, idx_d, lab_d), keep):
        assert torch.equal(_bits(t), _bits(was)), "an input was modified"
    assert torch.isnan(sbuf[m * c:]).all() and (pbuf[m * topn:] == -77).all() and (fbuf[1:] == -77).all(), "wrote past an output's end"
    if want_scores:
        assert not torch.isnan(sbuf[:m * c]).any(), "score elements never written"
    else:
        assert torch.isnan(sbuf).all()
    assert (pbuf[:m * topn] != -77).all()
    return pbuf[:m * topn].view(m, topn), sbuf[:m * c].view(m, c), int(fbuf[0].item())


@pytest.mark.parametrize("temperature", VOTE_TEMPERATURES)
@pytest.mark.parametrize("case", VOTE_CASES, ids=lambda c: "k%d-C%d-top%d" % c[:3])
def test_vote_against_fp64(case, temperature):
    k, c, topn, _ = case
    sim, idx, labels, _ = vote_inputs(case)
    it = kc.inv_temp32(temperature)
    ref64 = kc.vote_scores(sim, idx, labels, c, it)
    ref32 = kc.vote_scores_torch(sim, idx, labels, c, it, torch.float32).numpy()
    sim_d, idx_d, lab_d = _dev(sim), _dev(idx), _dev(labels, torch.int32)
    pred, scores, flag = _vote_abi(sim_d, idx_d, lab_d, c, topn, it)
    assert flag == 0
    got = scores.cpu().numpy()
    (eg, mg), (er, mr) = _err(got, ref64), _err(ref32, ref64)
    REPORT[f"k{k}-C{c}-top{topn}-T{temperature:g}"] = {"e_got": eg, "e_ref32": er, "m_got": mg, "m_ref32": mr, "ratio_e": _ratio(eg, er, FLOOR), "ratio_m": _ratio(mg, mr, FLOOR)}
    print(f"vote k={k} C={c} T={temperature:g}: e {eg:.3e} (ref32 {er:.3e}) m {mg:.3e} (ref32 {mr:.3e})")
    # pred: the stable arg-sort of the kernel's own scores, and the fp64 prediction wherever the fp64 margin is clear
    pred_np = pred.cpu().numpy().astype(np.int64)
    assert np.array_equal(pred_np, kc.top_classes(got, topn))
    margin = kc.relative_margin(ref64)
    clear = margin > kc.MU
    assert float((~clear).mean()) <= kc.MAX_EXCUSED
    assert np.array_equal(pred_np[clear, 0], kc.top_classes(ref64, 1)[clear, 0])
    # a second identical call: the same bits; without scores: the same predictions, nothing written
    pred2, scores2, _ = _vote_abi(sim_d, idx_d, lab_d, c, topn, it)
    assert torch.equal(pred2, pred) and torch.equal(_bits(scores2), _bits(scores))
    pred3, _, _ = _vote_abi(sim_d, idx_d, lab_d, c, topn, it, want_scores=False)
    assert torch.equal(pred3, pred)
    assert eg <= FACTOR * er + FLOOR and mg <= FACTOR * mr + FLOOR, (eg, er, mg, mr)


def test_vote_flags_and_refusals():
    from ssv_amd import ops
    from ssv_amd._lib import SsvError
    case = VOTE_CASES[1]
    sim, idx, labels, c = vote_inputs(case)
    it = kc.inv_temp32(0.07)
    want_pred = kc.top_classes(kc.vote_scores(sim, idx, labels, c, it), 1)
    pred, scores = ops.knn_vote(_dev(sim), _dev(idx), _dev(labels, torch.int32), c, 0.07, return_scores=True)
    assert pred.shape == (sim.shape[0], 1) and scores.shape == (sim.shape[0], c)
    assert np.array_equal(pred.cpu().numpy()[:, 0], want_pred[:, 0])
    assert torch.equal(ops.knn_vote(_dev(sim), _dev(idx), _dev(labels, torch.int32), c, 0.07), pred)
    for bad_idx, bad_label in ((len(labels), None), (-1, None), (None, c), (None, -1)):
        idx2, lab2 = idx.copy(), labels.copy()
        if bad_idx is not None:
            idx2[3, 4] = bad_idx
        else:
            lab2[idx[3, 4]] = bad_label
        with pytest.raises(SsvError, match="outside"):
            ops.knn_vote(_dev(sim), _dev(idx2), _dev(lab2, torch.int32), c, 0.07)
        _, got, flag = _vote_abi(_dev(sim), _dev(idx2), _dev(lab2, torch.int32), c, 1, it)          # raised and not counted
        ref = kc.vote_scores(sim, idx2, lab2, c, it)
        assert flag == 1 and np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * ref.max()
    nan_sim = sim.copy()
    nan_sim[5, 19] = np.nan                                          # the last place: a NaN ranks below every number
    _, got, flag = _vote_abi(_dev(nan_sim), _dev(idx), _dev(labels, torch.int32), c, 1, it)
    ref = kc.vote_scores(nan_sim, idx, labels, c, it)
    assert flag == 0 and np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * ref.max() and ref[5].sum() < kc.vote_scores(sim, idx, labels, c, it)[5].sum()
    with pytest.raises(SsvError):
        ops.knn_vote(_dev(sim), _dev(idx), _dev(labels, torch.int32), c, 0.07, topn=c + 1)          # topn > C
    with pytest.raises(SsvError):
        ops.knn_vote(_dev(sim), _dev(idx), _dev(labels, torch.int32), c, 0.07, topn=9)
    with pytest.raises(SsvError):
        ops.knn_vote(_dev(sim), _dev(idx), _dev(labels, torch.int32), c, 0.0)
    with pytest.raises(SsvError):
        ops.knn_vote(torch.as_tensor(sim), torch.as_tensor(idx), torch.as_tensor(labels, dtype=torch.int32), c, 0.07)      # CPU tensors


def test_search_refusals():
    from ssv_amd import _lib, ops
    from ssv_amd._lib import SsvError
    bank, _, queries, _ = kc.integers()
    bd, qd = _dev(bank), _dev(queries)
    for kwargs in ({"k": 0}, {"k": 1001}, {"k": 20, "chunk_rows": -1}, {"k": 20, "part_cols": -4}):
        with pytest.raises(SsvError):
            ops.knn_search(qd, bd, **kwargs)
    with pytest.raises(SsvError):
        ops.knn_search(qd, _dev(np.zeros((2000, 64), np.float32)), 1025)                              # k above the limit
    with pytest.raises(SsvError):
        ops.knn_search(qd, bd[:, :32].contiguous(), 5)                                                # another width
    with pytest.raises(SsvError):
        ops.knn_search(torch.as_tensor(queries), torch.as_tensor(bank), 5)                            # CPU tensors
    lib = _lib.load()
    out = torch.empty(300 * 20, dtype=torch.float32).cuda()
    oi = torch.empty(300 * 20, dtype=torch.int32).cuda()
    ws = torch.empty(4 << 20, dtype=torch.uint8).cuda()
    args = lambda m, n, d, k, cr=0, pc=0: (m, n, d, k, qd.data_ptr(), bd.data_ptr(), out.data_ptr(), oi.data_ptr(), 6, cr, pc, ws.data_ptr(), ws.numel(), _lib.stream())
    for bad in ((300, 1000, 64, 0), (300, 1000, 64, 1001), (300, 1000, 62, 20), (300, 1000, _lib.KNN_MAX_D + 4, 20), (-1, 1000, 64, 20), (300, 1 << 31, 64, 20),
                (1 << 20, 1000, 64, 20, 1 << 20, 0)):                                            # a chunk of S of 2^20 x 1000 floats
        assert lib.ssv_knn_search(*args(*bad)) == -1 and b"ssv_knn_search" in lib.ssv_last_error(), bad
        assert lib.ssv_knn_search_workspace_bytes(*bad[:4], 6, *(bad[4:] or (0, 0))) == 0
    small = torch.empty(1024, dtype=torch.uint8).cuda()
    assert lib.ssv_knn_search(300, 1000, 64, 20, qd.data_ptr(), bd.data_ptr(), out.data_ptr(), oi.data_ptr(), 6, 0, 0, small.data_ptr(), small.numel(), _lib.stream()) == -2
    # the default partition keeps the workspace bounded for a bank of ten million rows
    assert 0 < lib.ssv_knn_search_workspace_bytes(10000, 10_000_000, 128, 200, 6, 0, 0) <= (256 + 384 + 8 + 1) << 20
    assert 0 < lib.ssv_knn_search_workspace_bytes(10000, 10_000_000, 8192, 1024, 6, 0, 0) <= (256 + 384 + 8 + 1) << 20


# ====================================================================================================================== end to end
@pytest.mark.parametrize("arith", ARITHMETICS)
def test_knn_classify_on_integer_features(arith):
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    bank, yb, queries, yq = kc.integers()
    c = kc.INT_SHAPE[3]
    with ops.arithmetic(arith):
        for k in kc.KS + (bank.shape[0],):
            got = eval_utils.knn_classify(bank, yb, queries, yq, k=k, temperature=kc.INT_T, num_classes=c, normalize=False)
            want = kc.classify(bank, yb, queries, yq, k, kc.INT_T, c)
            pred = got["pred"].cpu().numpy().astype(np.int64)
            assert np.array_equal(pred[:, 0], want["pred"][:, 0]), k
            assert got["top1"] == want["top1"] == float(np.mean(pred[:, 0] == yq))
            assert got["top5"] == float(np.mean((pred == yq[:, None]).any(1)))
            # the hand composition: the same bits
            sim, idx = ops.knn_search(_dev(queries), _dev(bank), k)
            assert torch.equal(ops.knn_vote(sim, idx, _dev(yb, torch.int32), c, kc.INT_T, topn=5), got["pred"])


@pytest.mark.parametrize("index,arith", ((0, "bf16x3"), (0, "f32"), (1, "bf16x3")))
def test_knn_classify_on_fp32_features(index, arith):
    from ssv_amd import ops
    from ssv_amd.utils import eval_utils
    bank, yb, queries, yq = kc.blobs(index)
    m, n, _, c = kc.BLOB_SHAPES[index]
    it = kc.inv_temp32(kc.T_DEFAULT)
    s = kc.similarities(queries, bank)
    bound = 2 * kc.tau(queries, bank) / kc.T_DEFAULT + kc.MU
    with ops.arithmetic(arith):
        for k in kc.KS + ((n,) if index == 0 else ()):              # k = n is left out at (257, 1500, 36, 100): tests/test_knn_classify_cpu.py
            got = eval_utils.knn_classify(bank, yb, queries, yq, k=k, num_classes=c)
            bn, qn = ops.l2norm_fwd(_dev(bank))[0], ops.l2norm_fwd(_dev(queries))[0]
            sim, idx = ops.knn_search(qn, bn, k)
            assert torch.equal(ops.knn_vote(sim, idx, _dev(yb, torch.int32), c, kc.T_DEFAULT, topn=5), got["pred"])       # the hand composition: the same bits
            idx_np = idx.cpu().numpy().astype(np.int64)
            scores = kc.vote_scores(np.take_along_axis(s, idx_np, axis=1), idx_np, yb, c, it)       # the fp64 vote over the RETURNED list
            excused = kc.relative_margin(scores) <= bound
            pred = got["pred"].cpu().numpy().astype(np.int64)
            share = float(excused.mean())
            print(f"blobs {kc.BLOB_SHAPES[index]} {arith} k={k}: excused {share:.2%}, top1 {got['top1']:.4f} top5 {got['top5']:.4f}")
            assert share <= kc.MAX_EXCUSED
            assert np.array_equal(pred[~excused, 0], kc.top_classes(scores, 1)[~excused, 0])
            assert got["top1"] == float(np.mean(pred[:, 0] == yq)) and got["top5"] == float(np.mean((pred == yq[:, None]).any(1)))
    if n <= 1024:
        few = eval_utils.knn_classify(bank, yb % 3, queries, yq % 3, k=5000)                         # k is clipped to the bank; fewer than 5 classes
        assert few["top5"] is None and few["pred"].shape == (m, 3)
        assert torch.equal(few["pred"], eval_utils.knn_classify(bank, yb % 3, queries, yq % 3, k=n)["pred"])
    else:
        with pytest.raises(ops._lib.SsvError, match="1024"):                                         # clipped to the bank, which is above the search's limit: refused
            eval_utils.knn_classify(bank, yb % 3, queries, yq % 3, k=5000)


# ====================================================================================================================== trainer and command line
def test_main_knn_eval_from_a_checkpoint(tmp_path, monkeypatch):
    """`-t knn_eval -l <dir>` on a one-epoch synthetic resnet18 checkpoint logs the line; knn_classify_validate() returns the same numbers."""
    from ssv_amd import main as cli
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "simclr.yaml")))
    cfg["epochs"], cfg["eval_every"] = 1, 1
    cfg["data"]["batch_size"] = 32
    cfg["data"]["synthetic"] = {"num_train": 64, "num_test": 48, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"]["epochs"] = 1
    cfg["knn_eval"] = {"k": 10, "temperature": 0.1}
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    cli.main(["-c", str(path), "-a", "simclr", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "simclr" / "resnet18" / "run"
    assert (out / "best_model.pt").exists()
    model = cli.main(["-c", str(path), "-a", "simclr", "-m", "resnet18", "-t", "knn_eval", "-o", "knn", "-l", str(out)])
    log = (tmp_path / "outputs" / "simclr" / "resnet18" / "knn" / "trainlogs.txt").read_text()
    lines = [ln for ln in log.splitlines() if "Test kNN classifier accuracy:" in ln]
    assert len(lines) == 1
    top1, top5 = (float(v) for v in lines[0].split("top-1 ")[1].split(" top-5 "))
    res = model.knn_classify_validate()
    assert res["pred"].shape == (48, 5) and 0.0 <= res["top1"] <= res["top5"] <= 1.0
    assert "{:.4f} {:.4f}".format(res["top1"], res["top5"]) == "{:.4f} {:.4f}".format(top1, top5)
    # the same call by hand on the model's own features
    from ssv_amd.utils import eval_utils
    by_hand = eval_utils.knn_classify(*model.build_features("train"), *model.build_features("test"), k=10, temperature=0.1, num_classes=10)
    assert by_hand["top1"] == res["top1"] and torch.equal(by_hand["pred"], res["pred"])
