"""GPU: every launch form of csrc/nnlookup.hip - ssv_nn_lookup straight through the C ABI on guarded buffers - against an fp64 search on the same fp32 inputs
(tests/nnclr_oracle.py: lookup_inputs / lookup_reference on FORM_LOOKUP_CASES), in BOTH arithmetics (bf16x3: nn_prep_k, nn_fused_k<KT>, nn_fold_k where the width
allows it; f32, and bf16x3 at the other widths: the GEMM through the workspace, nn_rowarg_k, nn_fold_k).  tests/test_nnclr_cpu.py restates the launch plan
(nnclr_oracle.lookup_plan), holds it against ssv_nn_lookup_workspace_bytes and ops.nn_lookup_slice_rows, proves without a GPU that every case below reaches the
form its label names and that no case excuses more than 1 % of its rows, and keeps this table honest.

Held for every case, the rule of tests/test_gpu_nnclr.py::test_lookup_against_fp64: with s64 = Q B^T in float64 and tau_i = 2^-14 |q_i| max_j |b_j|, a row whose
fp64 margin is at least tau_i carries the fp64 first arg-max EXACTLY, a row below it an index whose fp64 score is within tau_i of the best;
|sim - s64[idx]| <= tau_i; nn is out_scale * bank[idx] bit for bit.  nn, idx, sim and the workspace (ssv_nn_lookup_workspace_bytes bytes exactly) are views with
1024 guard elements behind them; the call runs twice - workspace prefilled with 0xA5 and out_scale 1, workspace prefilled with 0x00 and out_scale 10 - and idx
and sim carry equal bits; no output element keeps its prefill, every guard is untouched, the queries and the bank are bit-identical afterwards.

Branch labels (label, entry point, the shape (m, n, d), what the case reaches):

  fused.kt4_ragged     ssv_nn_lookup  (96, 600, 32)       nn_fused_k<4> with T = 3: the fourth tile repeats the third and is not written; two slices, the second ragged
  fused.kt4_full       ssv_nn_lookup  (128, 1299, 96)     nn_fused_k<4> with T = 4; three slices; d % 64 = 32: the upper half of the second chunk is zeros
  fused.nch16          ssv_nn_lookup  (70, 300, 1024)     SSV_NN_LOOKUP_FUSED_MAX_D: 16 chunk trips of the fragment ring at STEPS = 16
  unfused.d36          ssv_nn_lookup  (40, 300, 36)       d % 32 != 0: the GEMM route under bf16x3 as under f32
  unfused.wide         ssv_nn_lookup  (40, 300, 1056)     d above the fused limit: the GEMM route under bf16x3 as under f32
  fused.kt8_tail       ssv_nn_lookup  (1030, 200, 32)     33 tiles: five blocks of nn_fused_k<8>, the last with one live tile (bf16x3)
  unfused.two_chunks   ssv_nn_lookup  (1030, 200, 32 / 36)  m > 1024: a second query chunk of 6 rows, row0 = 1024 in nn_rowarg_k (f32 at d = 32, both at d = 36)
  fused.long_slice     ssv_nn_lookup  (8, 2^21 + 600, 32)  L = 1024 with 2049 slices: a wave's quarter is 256 rows, the last slice holds 600 (bf16x3)
  unfused.parts        ssv_nn_lookup  (8, 2^21 + 600, 32)  33 parts of the bank folded into the running best (f32)
  planted.kt4          ssv_nn_lookup  (128, 1299, 96)     one planted bank row for queries 0, 31, 32, 63, 64, 95, 96 and 127 - lanes 0 and 31 of each of the four tiles - at the quarter and slice boundaries
  planted.tie          ssv_nn_lookup  (128, 1299, 96)     query 100 (tile 3) planted on both sides of the boundary between slices 1 and 2: the lower index wins, and with it removed the upper one wins with the same bits
  buffers.guarded      ssv_nn_lookup  every case: guards, prefills, inputs
  det.workspace        ssv_nn_lookup  every case: equal bits over the two workspace prefills

No FACTOR here: the lookup's tolerance is tau.  Measured on an MI355X (profiles/lookup_loss_forms_report.json, "lookup", written under
SSV_LOOKUP_LOSS_FORMS_REPORT=<path>): over the 64 runs of the table and the planted case not one row off the fp64 arg-max in either arithmetic - the excused rows
included: 6 of 1030 at worst, 1030 x 200 x 36 clustered - and |sim - s64| at most 0.008 tau (40 x 300 x 1056 clustered under f32).
"""
import re

import numpy as np
import pytest
import torch

import forms_report as fr
import nnclr_oracle as no

pytestmark = pytest.mark.gpu
ARITHS = ("bf16x3", "f32")
FILLS = (-1515870811, 0)                                                 # 0xA5A5A5A5 and 0x00000000 as the int32 prefill of the workspace
UNWRITTEN = -5                                                           # the prefill of idx: no index
REPORT = {}                                                              # per run: rows off the fp64 arg-max, rows excused, the worst |sim - s64| / tau

# case id -> labels per arithmetic (bf16x3, f32)
CASE_LABELS = {
    "96x600x32": ("fused.kt4_ragged", ""),
    "128x1299x96": ("fused.kt4_full", ""),
    "70x300x1024": ("fused.nch16", ""),
    "40x300x36": ("unfused.d36", "unfused.d36"),
    "40x300x1056": ("unfused.wide", "unfused.wide"),
    "1030x200x32": ("fused.kt8_tail", "unfused.two_chunks"),
    "1030x200x36": ("unfused.two_chunks", "unfused.two_chunks"),
    f"8x{no.FORM_BIG_N}x32": ("fused.long_slice", "unfused.parts"),
}
TARGETS = {"test_lookup_forms_against_fp64": " ".join(sorted({l for pair in CASE_LABELS.values() for l in pair if l})) + " buffers.guarded det.workspace",
           "test_planted_winners_in_every_tile_of_four": "planted.kt4 planted.tie"}


def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(ssv_\w+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def reaches(label, m, n, d, arith):
    """Whether the launch plan of (m, n, d) under `arith` is the form `label` names (tests/test_nnclr_cpu.py runs this for every case without a GPU)."""
    p = no.lookup_plan(m, n, d, arith)
    if label.startswith("fused.") != p["fused"]:
        return False
    return {"fused.kt4_ragged": lambda: p["KT"] == 4 and p["T"] == 3 and p["P"] > 1,
            "fused.kt4_full": lambda: p["KT"] == 4 and p["T"] == 4 and p["P"] >= 3 and d % 64 == 32,
            "fused.nch16": lambda: p["nch"] == 16 and d == no.FUSED_MAX_D,
            "fused.kt8_tail": lambda: p["KT"] == 8 and p["blocks"] > 1 and p["T"] % 8 == 1,
            "fused.long_slice": lambda: p["L"] == 2 * no.SLICE and p["P"] > no.MAX_SLICES // 2 and n % p["L"] != 0,
            "unfused.d36": lambda: d % 32 != 0 and d < no.FUSED_MAX_D,
            "unfused.wide": lambda: d % 32 == 0 and d > no.FUSED_MAX_D,
            "unfused.two_chunks": lambda: p["chunks"] == 2 and m % no.CHUNK_ROWS != 0,
            "unfused.parts": lambda: p["parts"] > 1}[label]()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from ssv_amd import _lib
    yield _lib.load()
    fr.write([], env="SSV_LOOKUP_LOSS_FORMS_REPORT", sha_key="source_sha16", extra={"lookup": REPORT})


def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


def _lookup(lib, q, bank, n, arith, scale, fill, what):
    """ssv_nn_lookup on guarded buffers: q [m, d] and bank [n, d] float32 numpy -> (nn [m, d] float32, idx int64, sim float32) numpy"""
    from ssv_amd import _lib
    P = _lib.ptr
    m, d = q.shape
    buf = fr.Buffers()
    qd, bd = buf.up("queries", q), buf.up("bank", bank)
    nn = buf.out("nn", m * d, torch.float32, float("nan"))
    idx = buf.out("idx", m, torch.int32, UNWRITTEN)
    sim = buf.out("sim", m, torch.float32, float("nan"))
    nbytes = int(lib.ssv_nn_lookup_workspace_bytes(m, n, d, _code(arith)))
    assert nbytes == no.lookup_plan(m, n, d, arith)["bytes"] and nbytes % 256 == 0
    ws = buf.out("ws", nbytes // 4, torch.int32, fill)
    assert all(t.data_ptr() % 16 == 0 for t in (qd, bd, nn, idx, sim, ws))
    _lib.call("ssv_nn_lookup", m, n, d, P(qd), P(bd), no.f32(scale), P(nn), P(idx), P(sim), _code(arith), P(ws), nbytes, _lib.stream())
    buf.verify(what)
    i = idx.cpu().numpy().astype(np.int64)
    assert ((i >= 0) & (i < n)).all(), f"{what}: an index outside [0, n) (or never written)"
    assert not bool(torch.isnan(nn).any()) and not bool(torch.isnan(sim).any()), f"{what}: nn or sim was not written everywhere"
    return nn.view(m, d).cpu().numpy(), i, sim.cpu().numpy()


def _gathered(bank, idx, scale):
    """out_scale * bank[idx] as one fp32 multiply per element, on the CPU"""
    return (np.float32(no.f32(scale)) * bank[idx]).astype(np.float32)


def _hold(what, r, bank, runs):
    """The rule of test_lookup_against_fp64 on the runs [(scale, (nn, idx, sim))] of one case; r: the reference dictionary of nnclr_oracle.lookup_reference."""
    rows = np.arange(r["s"].shape[0])
    for scale, (nn, idx, sim) in runs:
        wrong = idx != r["idx"]
        s_at = r["s"][rows, idx]
        err = np.abs(sim.astype(np.float64) - s_at)
        REPORT[f"{what} scale {scale:g}"] = {"rows": int(len(idx)), "off_the_fp64_argmax": int(wrong.sum()), "excused": int(r["excused"].sum()),
                                            "worst_sim_error_over_tau": float((err / r["tau"]).max())}
        print(f"{what} scale {scale:g}: {int(wrong.sum())} of {len(idx)} rows off the fp64 arg-max ({int(r['excused'].sum())} excused), max |sim - s64| / tau "
              f"{(err / r['tau']).max():.3g}")
        assert not (wrong & ~r["excused"]).any(), f"{what}: rows {np.nonzero(wrong & ~r['excused'])[0][:8]} carry another index than the fp64 arg-max"
        assert (r["best"] - s_at <= r["tau"]).all(), f"{what}: an excused row's index scores more than tau below the best"
        assert (err <= r["tau"]).all(), f"{what}: sim is more than tau from the fp64 score at the chosen index"
        assert np.array_equal(nn.view(np.int32), _gathered(bank, idx, scale).view(np.int32)), f"{what}: nn is not out_scale * bank[idx] bit for bit"
    (_, (_, i0, s0)), (_, (_, i1, s1)) = runs
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.int32), s1.view(np.int32)), f"{what}: idx or sim changed with the workspace prefill or out_scale"


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(no.FORM_LOOKUP_CASES))
def test_lookup_forms_against_fp64(lib, name, arith):
    c = no.FORM_LOOKUP_CASES[name]
    label = CASE_LABELS[f"{c.m}x{c.n}x{c.d}"][ARITHS.index(arith)]
    assert not label or reaches(label, c.m, c.n, c.d, arith), f"{name}[{arith}] does not reach {label}"
    q, b = no.lookup_inputs(name)
    r = no.lookup_reference(name)
    assert float(r["excused"].mean()) <= no.MAX_EXCUSED
    what = f"{name}[{arith}]"
    runs = [(scale, _lookup(lib, q, b, c.n, arith, scale, fill, what)) for scale, fill in zip((1.0, 10.0), FILLS)]
    _hold(what, r, b, runs)


def _planted(n, d, m, places, seed):
    """A Gaussian unit-norm bank [n, d] and m Gaussian unit-norm queries (float32 numpy); query k of `places` is copied into the bank at every index of places[k]"""
    g = torch.Generator().manual_seed(seed)
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    bank, q = unit(torch.randn(n, d, generator=g)), unit(torch.randn(m, d, generator=g))
    for k, js in places.items():
        for j in js:
            bank[j] = q[k]
    return q.numpy(), bank.numpy()


@pytest.mark.parametrize("arith", ARITHS)
def test_planted_winners_in_every_tile_of_four(lib, arith):
    from ssv_amd import ops
    m, n, d = 128, 1299, 96
    L = ops.nn_lookup_slice_rows(n)
    qr = L // 4                                                           # a wave's quarter of a slice
    assert L == no.lookup_plan(m, n, d, "bf16x3")["L"] and 2 * L + 2 * qr < n - 1 < 2 * L + 3 * qr and reaches("fused.kt4_full", m, n, d, "bf16x3")
    # lanes 0 and 31 of the four query tiles: the last row of a quarter and the first of the next, the last row of slice 0 and the first of slice 1, a quarter
    # boundary of the last slice, the first row of its ragged quarter and the last row of the bank; query 100 on both sides of the boundary of slices 1 | 2
    places = {0: [qr - 1], 31: [qr], 32: [L - 1], 63: [L], 64: [2 * L + qr - 1], 95: [2 * L + qr], 96: [2 * L + 2 * qr], 127: [n - 1], 100: [2 * L - 1, 2 * L]}
    q, bank = _planted(n, d, m, places, 21)
    s = no.scores(q, bank)
    t = no.tau(q, bank)
    two = -np.partition(-s, 1, axis=1)[:, :2]
    margin = two[:, 0] - two[:, 1]
    ref = {"s": s, "idx": s.argmax(1), "best": two[:, 0], "margin": margin, "tau": t, "excused": margin < t}
    ref["excused"][100] = False                                            # an exact tie: the FIRST arg-max is required, and numpy's argmax gives it
    assert all(ref["idx"][k] == js[0] for k, js in places.items()) and int(ref["excused"].sum()) <= 1
    what = f"planted[{arith}]"
    runs = [(scale, _lookup(lib, q, bank, n, arith, scale, fill, what)) for scale, fill in zip((1.0, 10.0), FILLS)]
    _hold(what, ref, bank, runs)
    idx, sim = runs[0][1][1], runs[0][1][2]
    assert {k: int(idx[k]) for k in places} == {k: js[0] for k, js in places.items()}
    assert np.abs(sim[list(places)] - 1.0).max() < 1e-5
    # bit-identical rows score bit-identically on either side of the slice boundary: with the first copy removed the second wins with the same bits
    bank2 = bank.copy()
    bank2[2 * L - 1] = 0.0
    _, idx2, sim2 = _lookup(lib, q, bank2, n, arith, 1.0, FILLS[0], what + " (first copy removed)")
    assert idx2[100] == 2 * L and sim2[100:101].view(np.int32) == sim[100:101].view(np.int32)
    keep = (np.arange(m) != 100) & (idx != 2 * L - 1)
    assert np.array_equal(idx2[keep], idx[keep]) and np.array_equal(sim2[keep].view(np.int32), sim[keep].view(np.int32))
