"""GPU: the two kernels of DenseCL's dense term (csrc/densecl.hip: ssv_queue_nce, ssv_dense_match) straight through the C ABI on NaN-guarded outputs and a
0xA5-guarded workspace, against tests/densecl_oracle.py (fp64, plain torch under autograd) on the same fp32 inputs, in both arithmetics.

ssv_queue_nce: accuracy at every case of densecl_oracle.cases() (m in {1, 33, 70} and just past every m-threshold of the plan, the fused widths 32 .. 128 and the
unfused 4, 36, 160, K in {1, 31, 33, 513, 640}; the variants plain, same, late, dup, zero), equal bits over a differently filled workspace, untouched guards and
inputs, rows behind K / m / mk never read (they hold NaN), the device flag, every refusal of the limits list, and the fused against the unfused route.
The `dup` variant plants one row on both sides of the slice boundary at row 256.  A bank row's score is one instruction sequence wherever the row sits, but the
contract has no output that isolates it (lse and dq sum over the slices in their order), so the variant is held to the accuracy rule and to equal bits between
two calls, and - since both copies score alike - to a loss that does not change when the two rows are exchanged with each other.

ssv_dense_match: idx equals the fp64 arg-max in every cell except cells where the fp64 cosine of the chosen cell is within 8 * 2^-24 of the best (at most 1 % of
a case's cells; tests/test_densecl_cpu.py shows that the fp32 reference itself needs no excuse), sim under the accuracy rule, the planted exact tie, the all-zero
rows, guards, refusals and untouched inputs.

Accuracy.  The project's rule.  With ref64 = the oracle in float64 on the CPU, ref32 = the same lines in float32, e(x) = |x - ref64|_2 / |ref64|_2 and
m(x) = max|x - ref64| / max|ref64|, for loss, lse, dq and sim of every case:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
FLOOR = 2 * 2^-24.  FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured on an MI355X against ref32
(profiles/dense_nce_kernels_report.json, written by this file under SSV_DENSE_NCE_REPORT=<path>), rounded up to the next power of two and never above 8.
The cases keep the mean probability of the positive below 0.9 and every |score| below 60 (tests/test_densecl_cpu.py), so ref32 itself is meaningful."""
import ctypes as C
import json
import os

import pytest
import torch

import densecl_oracle as do
from densecl_oracle import FACTOR, FLOOR

pytestmark = pytest.mark.gpu
GUARD = 1024
REPORT = {}
INVALID = -1                                              # SSV_ERR_INVALID
ARITHS = ("bf16x3", "f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_DENSE_NCE_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """n floats of NaN with GUARD floats of NaN behind them (as int32 the NaN is 0x7fc00000: no flag or index the kernels write)"""

    def __init__(self, n, dev):
        self.n, self.buf = n, torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def t(self):
        return self.buf[:self.n]

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool(torch.isnan(self.buf[self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


class Scratch:
    """the workspace: ``fill`` bytes, with 4 * GUARD bytes of 0xA5 behind them"""

    def __init__(self, nbytes, dev, fill=0xA5):
        self.nbytes = int(nbytes)
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[:self.nbytes] = fill

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _tail(t, dev, rows=8):
    """``t`` on the device as the head of a larger buffer whose tail holds NaN (int32: -1): what lies behind m, mk and K must never enter a result"""
    pad = torch.full((rows,) + tuple(t.shape[1:]), float("nan") if t.dtype == torch.float32 else -1, dtype=t.dtype)
    big = torch.cat([t, pad]).to(dev)
    return big, big[:t.shape[0]]


def _call(q, keys, pos, bank, K, inv_temp, arith, dev, fill=0xA5):
    """ssv_queue_nce through the C ABI on guarded buffers: CPU tensors in -> {loss, lse, dq (fp32), flag (int)} on the CPU"""
    from ssv_amd import _lib
    (m, d), mk = q.shape, keys.shape[0]
    bigs, ins = zip(*(_tail(t, dev) for t in (q, keys, pos, bank)))
    before = [b.clone() for b in bigs]
    loss, lse, dq, flag = Out(1, dev), Out(m, dev), Out(m * d, dev), Out(1, dev)
    ws = Scratch(_lib.load().ssv_queue_nce_workspace_bytes(m, K, d, _code(arith)), dev, fill)
    _lib.call("ssv_queue_nce", m, d, K, mk, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), float(inv_temp), loss.ptr(), lse.ptr(), dq.ptr(),
              flag.ptr(), _code(arith), ws.ptr(), ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    assert loss.guard_ok() and lse.guard_ok() and dq.guard_ok() and flag.guard_ok(), "an output guard was written"
    for a, b in zip(bigs, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was written"
    return {"loss": loss.t.cpu().reshape(()), "lse": lse.t.cpu(), "dq": dq.t.view(m, d).cpu(), "flag": int(flag.t.view(torch.int32).cpu()[0])}


# ---- accuracy against fp64 --------------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _refs(case):
    """the inputs, the fp64 oracle and its fp32 evaluation, computed once per case and never modified"""
    if case not in _REFS:
        ins = do.make_case(case)
        _REFS[case] = (ins, do.queue_nce(*ins, dtype=torch.float64), do.queue_nce(*ins, dtype=torch.float32))
    return _REFS[case]


def _figures(got, ref64, ref32):
    e, m = do.errs(got, ref64)
    e32, m32 = do.errs(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32, fails, bound=1.0):
    f = REPORT[f"{name}.{what}"] = _figures(got.detach().cpu(), ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})  ratios {f['ratio_e']:.3g} {f['ratio_m']:.3g}")
    if not (f["e"] <= bound * (FACTOR * f["e_ref32"] + FLOOR) and f["m"] <= bound * (FACTOR * f["m_ref32"] + FLOOR)):
        fails.append((name, what, f))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", do.cases(), ids=do.case_id)
def test_queue_nce_against_fp64(dev, case, arith):
    ins, r64, r32 = _refs(case)
    got = _call(*ins, arith, dev, 0xA5)
    again = _call(*ins, arith, dev, 0x00)
    assert got["flag"] == 0
    for k in ("loss", "lse", "dq"):
        assert not bool(torch.isnan(got[k]).any()), f"{k} was not written everywhere"
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{k} depends on what the workspace held"
    tag = f"{do.case_id(case)}[{arith}]"
    fails = []
    for k in ("loss", "lse", "dq"):
        _hold(tag, k, got[k], r64[k], r32[k], fails)
    assert not fails, fails
    if case[3] == "dup":                                  # the two copies are one row: exchanging them is the same call
        q, keys, pos, bank, K, it = ins
        swapped = bank.clone()
        swapped[255], swapped[256] = bank[256], bank[255]
        other = _call(q, keys, pos, swapped, K, it, arith, dev)
        for k in ("loss", "lse", "dq"):
            assert torch.equal(_bits(other[k]), _bits(got[k])), k


# ---- the contract cases -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("d", [64, 36])
def test_a_bad_positive_sets_the_flag_and_stays_in_bounds(dev, d, arith):
    q, keys, pos, bank, K, it = do.make_case((70, d, 640, "plain"))
    mk = keys.shape[0]
    assert _call(q, keys, pos, bank, K, it, arith, dev)["flag"] == 0
    for bad in (-1, mk, 1 << 30):
        for row in (5, 69):
            p = pos.clone()
            p[row] = bad
            assert _call(q, keys, p, bank, K, it, arith, dev)["flag"] == 1, (bad, row)      # _call checks every guard and every input


def test_every_refusal_leaves_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    lib.ssv_last_error.restype = C.c_char_p
    m, d, K = 16, 32, 40
    q, keys, pos, bank, _, it = do.make_case((m, d, K, "plain"))
    mk = keys.shape[0]
    qd, kd, pd, bd = q.to(dev), keys.to(dev), pos.to(dev), bank.to(dev)
    ws_ok = int(lib.ssv_queue_nce_workspace_bytes(m, K, d, _lib.ARITH_BF16X3))

    def refused(what, m=m, d=d, K=K, mk=mk, it=it, arith=_lib.ARITH_BF16X3, ws_bytes=None, shift=None, alias=None, null=None):
        loss, lse, dq, flag = Out(1, dev), Out(max(m, 1), dev), Out(max(m, 1) * max(d, 4), dev), Out(1, dev)
        ws = Scratch(max(ws_ok, 1 << 20), dev)
        args = {"q": qd.data_ptr(), "keys": kd.data_ptr(), "pos": pd.data_ptr(), "bank": bd.data_ptr(), "loss": loss.ptr(), "lse": lse.ptr(), "dq": dq.ptr(),
                "flag": flag.ptr(), "ws": ws.ptr()}
        if shift:
            args[shift] += 4
        if alias:
            args[alias[0]] = args[alias[1]]
        if null:
            args[null] = None
        rc = lib.ssv_queue_nce(m, d, K, mk, args["q"], args["keys"], args["pos"], args["bank"], it, args["loss"], args["lse"], args["dq"], args["flag"], arith, args["ws"],
                               ws.nbytes if ws_bytes is None else ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        assert rc == INVALID, (what, rc)
        assert lib.ssv_last_error().decode().startswith("ssv_queue_nce:"), (what, lib.ssv_last_error())
        assert loss.untouched() and lse.untouched() and dq.untouched() and flag.untouched() and ws.guard_ok(), f"{what}: an output was touched"
        assert bool((ws.buf == 0xA5).all()), f"{what}: the workspace was touched"

    refused("m = 0", m=0)
    refused("m above the limit", m=do.MAX_M + 1)
    refused("K = 0", K=0)
    refused("K = 2^31", K=1 << 31)
    refused("mk = 0", mk=0)
    refused("mk = 2^31", mk=1 << 31)
    refused("d no multiple of 4", d=30)
    refused("d = 0", d=0)
    refused("d above the limit", d=8196)
    for bad in (0.0, -5.0, float("inf"), float("nan")):
        refused(f"inv_temp {bad}", it=bad)
    refused("an unknown arithmetic", arith=5)
    refused("a short workspace", ws_bytes=ws_ok - 1)
    for name in ("q", "keys", "pos", "bank", "loss", "lse", "dq", "flag", "ws"):
        refused(f"{name} misaligned", shift=name)
        refused(f"{name} NULL", null=name)
    refused("dq aliases q", alias=("dq", "q"))
    refused("dq aliases the bank", alias=("dq", "bank"))
    refused("lse aliases the workspace", alias=("lse", "ws"))
    refused("loss aliases flag", alias=("loss", "flag"))
    # and the same arguments unchanged are accepted
    got = _call(q, keys, pos, bank, K, it, "bf16x3", dev)
    assert got["flag"] == 0 and bool(torch.isfinite(got["dq"]).all())


@pytest.mark.parametrize("case", do.ROUTES_AGREE, ids=do.case_id)
def test_the_fused_and_the_unfused_route_agree(dev, case):
    """bf16x3 takes the fused kernel at these widths, f32 the GEMM route: each holds the rule against fp64 (above), so they differ by at most twice its bound"""
    m, d, K, _ = case
    assert do.plan(m, K, d, "bf16x3")["fused"] and not do.plan(m, K, d, "f32")["fused"]
    ins, r64, r32 = _refs(case)
    fused, unfused = _call(*ins, "bf16x3", dev), _call(*ins, "f32", dev)
    fails = []
    for k in ("loss", "lse", "dq"):
        e, mx = do.errs(fused[k], unfused[k])
        e32, m32 = do.errs(r32[k], r64[k])
        print(f"{do.case_id(case)}.{k}: fused against unfused e {e:.3g} m {mx:.3g} (ref32 {e32:.3g} {m32:.3g})")
        if not (e <= 2 * (FACTOR * e32 + FLOOR) and mx <= 2 * (FACTOR * m32 + FLOOR)):
            fails.append((k, e, mx, e32, m32))
    assert not fails, fails


# ---- ssv_dense_match ----------------------------------------------------------------------------------------------------------------------------------------------
def _match(f1, f2, arith, dev, eps=1e-12):
    from ssv_amd import _lib
    b, s, c = f1.shape
    bigs, ins = zip(*(_tail(t, dev, rows=1) for t in (f1, f2)))
    before = [x.clone() for x in bigs]
    idx, sim = Out(b * s, dev), Out(b * s, dev)
    _lib.call("ssv_dense_match", b, s, c, ins[0].data_ptr(), ins[1].data_ptr(), eps, idx.ptr(), sim.ptr(), _code(arith), _lib.stream())
    torch.cuda.synchronize()
    assert idx.guard_ok() and sim.guard_ok(), "an output guard was written"
    for a, x in zip(bigs, before):
        assert torch.equal(a.view(torch.int32), x.view(torch.int32)), "an input was written"
    return idx.t.view(torch.int32).view(b, s).cpu().long(), sim.t.view(b, s).cpu()


_MATCH_REFS = {}


def _match_refs(case):
    if case not in _MATCH_REFS:
        f1, f2 = do.make_match_case(case)
        _MATCH_REFS[case] = ((f1, f2), do.dense_match(f1, f2), do.dense_match(f1, f2, dtype=torch.float32))
    return _MATCH_REFS[case]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", do.MATCH_CASES, ids=do.match_id)
def test_dense_match_against_fp64(dev, case, arith):
    (f1, f2), r64, r32 = _match_refs(case)
    b, s, c, variant = case
    idx, sim = _match(f1, f2, arith, dev)
    base = s * torch.arange(b)[:, None]
    assert bool(((idx >= base) & (idx < base + s)).all()), "an index left its image"
    j = idx - base
    wrong = j != r64["j"]
    chosen, best = r64["cos"].gather(2, j[:, :, None])[:, :, 0], r64["cos"].max(dim=2).values
    excused = wrong & (best - chosen <= do.TIE)
    print(f"{do.match_id(case)}[{arith}]: {int(wrong.sum())} of {b * s} cells differ from the fp64 arg-max, {int(excused.sum())} within {do.TIE:.3g} of the best")
    assert bool((wrong == excused).all()), f"cells that chose a worse match: {wrong.nonzero().tolist()[:8]}"
    assert int(excused.sum()) <= 0.01 * b * s
    fails = []
    ok = ~wrong                                            # sim is the cosine of the CHOSEN pair: compare it where the pair is the reference's
    _hold(f"match-{do.match_id(case)}[{arith}]", "sim", sim[ok], r64["sim"][ok], r32["sim"][ok], fails)
    assert not fails, fails
    if variant == "planted":
        tied = r64["j"][0] == 3                            # cells of image 0 whose best match is the duplicated cell (cell 0 is one by construction): 3, never its copy 7
        assert bool(tied[0]) and bool((j[0][tied] == 3).all()) and not bool((j[0] == 7).any())
        assert int(j[b - 1, 1]) == 0 and float(sim[b - 1, 1]) == 0.0          # an all-zero f1 row
        assert not bool((j[b - 1][torch.arange(s) != 1] == 2).any())          # an all-zero f2 row is never chosen over a positive score


def test_dense_match_refusals_leave_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    lib.ssv_last_error.restype = C.c_char_p
    b, s, c = 2, 16, 64
    f1, f2 = (t.to(dev) for t in do.make_match_case((b, s, c, "plain")))

    def refused(what, b=b, s=s, c=c, eps=1e-12, arith=_lib.ARITH_BF16X3, shift=None, alias=None, null=None):
        idx, sim = Out(64, dev), Out(64, dev)
        args = {"f1": f1.data_ptr(), "f2": f2.data_ptr(), "idx": idx.ptr(), "sim": sim.ptr()}
        if shift:
            args[shift] += 4
        if alias:
            args[alias[0]] = args[alias[1]]
        if null:
            args[null] = None
        rc = lib.ssv_dense_match(b, s, c, args["f1"], args["f2"], eps, args["idx"], args["sim"], arith, _lib.stream())
        torch.cuda.synchronize()
        assert rc == INVALID, (what, rc)
        assert lib.ssv_last_error().decode().startswith("ssv_dense_match:"), (what, lib.ssv_last_error())
        assert idx.untouched() and sim.untouched(), f"{what}: an output was touched"

    refused("b = 0", b=0)
    refused("s = 0", s=0)
    refused("s above the limit", s=do.MATCH_MAX_S + 1)
    refused("c no multiple of 4", c=62)
    refused("c = 0", c=0)
    refused("c above the limit", c=8196)
    refused("b * s = 2^31", b=1 << 23, s=256)
    refused("eps = 0", eps=0.0)
    refused("an unknown arithmetic", arith=5)
    for name in ("f1", "f2", "idx", "sim"):
        refused(f"{name} misaligned", shift=name)
        refused(f"{name} NULL", null=name)
    refused("idx aliases sim", alias=("idx", "sim"))
    refused("sim aliases f1", alias=("sim", "f1"))
    idx, sim = _match(f1.cpu(), f2.cpu(), "bf16x3", dev)
    assert bool(torch.isfinite(sim).all())
