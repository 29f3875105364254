"""GPU: the ProtoNCE kernel of PCL (csrc/protonce.hip: ssv_proto_nce) straight through the C ABI on NaN-guarded outputs and a 0xA5-guarded workspace, against
tests/pcl_oracle.py (fp64, plain torch under autograd) on the same fp32 inputs, in both arithmetics: accuracy at every case of pcl_oracle.cases(), equal bits over
a differently filled workspace, untouched guards and inputs, rows behind ktot and behind m never read, the one-prototype segment, the device flag, every refusal
of the limits list, and the fused against the unfused route.

Accuracy.  The rule of tests/test_gpu_wmse.py.  With ref64 = the oracle in float64 on the CPU, ref32 = the same lines in float32, e(x) = |x - ref64|_2 / |ref64|_2
and m(x) = max|x - ref64| / max|ref64|, for loss, lse and dq of every case:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
FLOOR = 2 * 2^-24.  FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured on an MI355X against ref32
(profiles/proto_nce_kernels_report.json, written by this file under SSV_PROTO_NCE_REPORT=<path>), rounded up to the next power of two and never above 8.
The cases keep the mean probability of the positive below 0.9 and every |score| below 60 (tests/test_pcl_cpu.py), so ref32 itself is meaningful.
Measured (490 figures): 2.85 at worst - e and m of dq at m = 1, d = 36 over the segments (1, 33), the unfused route, the same in both arithmetics - then 2.00 for dq
at 70 x 32 over (513) under f32; the fused route (bf16x3 at 32, 64 and 128 columns) stays below 0.87 - so FACTOR is 4 (tests/pcl_oracle.py)."""
import ctypes as C
import json
import os

import pytest
import torch

import pcl_oracle as po
from pcl_oracle import FACTOR, FLOOR

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
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
    path = os.environ.get("SSV_PROTO_NCE_REPORT")
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
    """n floats of NaN with GUARD floats of NaN behind them (as int32 the NaN is 0x7fc00000: no flag the kernels write)"""

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
    """``t`` on the device as the head of a larger buffer whose tail holds NaN (int32: -1): what lies behind m and behind ktot must never enter a result"""
    pad = torch.full((rows,) + tuple(t.shape[1:]), float("nan") if t.dtype == torch.float32 else -1, dtype=t.dtype)
    big = torch.cat([t, pad]).to(dev)
    return big, big[:t.shape[0]]


def _call(q, protos, inv_phi, labels, seg_end, arith, dev, fill=0xA5):
    """ssv_proto_nce through the C ABI on guarded buffers: CPU tensors in -> {loss, lse, dq (fp32), flag (int)} on the CPU"""
    from ssv_amd import _lib
    (m, d), segs, ktot = q.shape, len(seg_end), seg_end[-1]
    bigs, ins = zip(*(_tail(t, dev) for t in (q, protos, inv_phi)))
    # labels [segs][m] is dense: rows behind m do not exist between its segments, only behind the last one
    lab_big = torch.cat([labels.flatten(), torch.full((64,), -1, dtype=torch.int32)]).to(dev)
    before = [b.clone() for b in bigs] + [lab_big.clone()]
    loss, lse, dq, flag = Out(1, dev), Out(segs * m, dev), Out(m * d, dev), Out(1, dev)
    ws = Scratch(_lib.load().ssv_proto_nce_workspace_bytes(m, ktot, d, segs, _code(arith)), dev, fill)
    _lib.call("ssv_proto_nce", m, d, segs, (C.c_int64 * segs)(*seg_end), ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), lab_big.data_ptr(), loss.ptr(), lse.ptr(),
              dq.ptr(), flag.ptr(), _code(arith), ws.ptr(), ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    assert loss.guard_ok() and lse.guard_ok() and dq.guard_ok() and flag.guard_ok(), "an output guard was written"
    for a, b in zip(list(bigs) + [lab_big], before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was written"
    return {"loss": loss.t.cpu().reshape(()), "lse": lse.t.view(segs, m).cpu(), "dq": dq.t.view(m, d).cpu(), "flag": int(flag.t.view(torch.int32).cpu()[0])}


# ---- accuracy against fp64 --------------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _refs(case):
    """the inputs, the fp64 oracle and its fp32 evaluation, computed once per case and never modified"""
    if case not in _REFS:
        ins = po.make_case(case)
        _REFS[case] = (ins, po.proto_nce(*ins, dtype=torch.float64), po.proto_nce(*ins, dtype=torch.float32))
    return _REFS[case]


def _figures(got, ref64, ref32):
    e, m = po.errs(got, ref64)
    e32, m32 = po.errs(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32, fails, bound=1.0):
    f = REPORT[f"{name}.{what}"] = _figures(got.detach().cpu(), ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})  ratios {f['ratio_e']:.3g} {f['ratio_m']:.3g}")
    if not (f["e"] <= bound * (FACTOR * f["e_ref32"] + FLOOR) and f["m"] <= bound * (FACTOR * f["m_ref32"] + FLOOR)):
        fails.append((name, what, f))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", po.cases(), ids=po.case_id)
def test_proto_nce_against_fp64(dev, case, arith):
    ins, r64, r32 = _refs(case)
    got = _call(*ins, arith, dev, 0xA5)
    again = _call(*ins, arith, dev, 0x00)
    assert got["flag"] == 0
    for k in ("loss", "lse", "dq"):
        assert not bool(torch.isnan(got[k]).any()), f"{k} was not written everywhere"
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{k} depends on what the workspace held"
    tag = f"{po.case_id(case)}[{arith}]"
    fails = []
    for k in ("loss", "lse", "dq"):
        _hold(tag, k, got[k], r64[k], r32[k], fails)
    assert not fails, fails
    if case[3] == "dup":                                  # the two copies score bit-identically: naming one or the other as the positive changes no bit of lse or of the loss
        q, protos, inv_phi, labels, seg_end = ins
        lab2 = labels.clone()
        lab2[labels == 255] = 256
        lab2[0, 0] = 255
        lab1 = labels.clone()
        lab1[0, 0] = 256
        a, b = _call(q, protos, inv_phi, lab1, seg_end, arith, dev), _call(q, protos, inv_phi, lab2, seg_end, arith, dev)
        assert torch.equal(_bits(a["lse"]), _bits(got["lse"])) and torch.equal(_bits(b["lse"]), _bits(got["lse"]))
        assert torch.equal(_bits(a["loss"]), _bits(b["loss"])), "a duplicate across the slice boundary scored differently from its first copy"


# ---- the contract cases -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("d", [128, 36])
@pytest.mark.parametrize("m", [1, 70])
def test_a_one_prototype_segment(dev, m, d, arith):
    """K = 1: lse is the score (within the rule).  The loss lse - s_y and dq = (p - 1) v (v = inv_phi_y c_y, p = 1) are zero in fp64 and in the fp32 reference, so
    the rule has no |ref64| to measure against; each is measured against what cancels instead.  lse is the ROUNDED score while the exponent of p and the
    positive's term take the unrounded product (an fma), so |lse - s_y| and |p - 1| are at most one rounding of the score, 2^-24 |s|, and FLOOR allows two:
    |loss| <= FLOOR * max|s| and max|dq| <= FLOOR * max(1, max|s|) * max|v| / (segs m)  (the 1: the fused route forms p v on the matrix pipe from the bf16
    pieces of v - two accumulator roundings of v itself)."""
    q, protos, inv_phi, labels, seg_end = po.make_case((m, d, (1,), "plain"))
    r64, r32 = po.proto_nce(q, protos, inv_phi, labels, seg_end), po.proto_nce(q, protos, inv_phi, labels, seg_end, torch.float32)
    got = _call(q, protos, inv_phi, labels, seg_end, arith, dev)
    assert got["flag"] == 0
    fails = []
    _hold(f"one-m{m}-d{d}[{arith}]", "lse", got["lse"], r64["lse"], r32["lse"], fails)
    assert not fails, fails
    assert float(r64["loss"]) == 0.0 and float(r64["dq"].abs().max()) == 0.0
    vmax, smax = float((protos[0].double() * float(inv_phi[0])).abs().max()), float(r64["lse"].abs().max())
    bound_dq = FLOOR * max(1.0, smax) * vmax / m
    print(f"one-m{m}-d{d}[{arith}]: loss {float(got['loss']):g} (bound {FLOOR * smax:.3g})  max|dq| {float(got['dq'].abs().max()):.3g} (bound {bound_dq:.3g})")
    assert abs(float(got["loss"])) <= FLOOR * smax and float(got["dq"].abs().max()) <= bound_dq
    # beside another segment its contribution to dq is zero: the call over (1, 33) gives exactly half the gradient of the call over the 33 alone (1 / segs)
    q, protos, inv_phi, labels, seg_end = po.make_case((m, d, (1, 33), "plain"))
    both = _call(q, protos, inv_phi, labels, seg_end, arith, dev)
    alone = _call(q, protos[1:].contiguous(), inv_phi[1:].contiguous(), labels[1:].contiguous(), (33,), arith, dev)
    assert torch.equal(_bits(both["lse"][1]), _bits(alone["lse"][0]))
    args = (q, protos[1:], inv_phi[1:], labels[1:], (33,))
    _hold(f"one+33-m{m}-d{d}[{arith}]", "dq", 2.0 * both["dq"], po.proto_nce(*args)["dq"], po.proto_nce(*args, dtype=torch.float32)["dq"], fails)
    assert not fails, fails                               # twice the gradient over (1, 33) is the gradient over the 33 alone, within the rule


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("d", [64, 36])
def test_bad_device_data_sets_the_flag_and_stays_in_bounds(dev, d, arith):
    case = (70, d, (7, 33, 600), "plain")
    q, protos, inv_phi, labels, seg_end = po.make_case(case)
    assert _call(q, protos, inv_phi, labels, seg_end, arith, dev)["flag"] == 0
    for bad in (7, -1, 600, 1 << 30):                      # just outside segment 0, negative, the size of the largest segment, far outside
        lab = labels.clone()
        lab[0, 5] = bad
        assert _call(q, protos, inv_phi, lab, seg_end, arith, dev)["flag"] == 1, bad      # _call checks every guard and every input
    lab = labels.clone()
    lab[2, 69] = 600
    assert _call(q, protos, inv_phi, lab, seg_end, arith, dev)["flag"] == 1
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        ip = inv_phi.clone()
        ip[40] = bad
        assert _call(q, protos, ip, labels, seg_end, arith, dev)["flag"] == 2, bad
    ip = inv_phi.clone()
    ip[639] = 0.0
    lab = labels.clone()
    lab[1, 0] = 33
    assert _call(q, protos, ip, lab, seg_end, arith, dev)["flag"] == 3


def test_every_refusal_leaves_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    lib.ssv_last_error.restype = C.c_char_p
    m, d, sizes = 16, 32, (40, 24)
    q, protos, inv_phi, labels, seg_end = po.make_case((m, d, sizes, "plain"))
    qd, cd, ipd, ld = q.to(dev), protos.to(dev), inv_phi.to(dev), labels.to(dev)
    ws_ok = int(lib.ssv_proto_nce_workspace_bytes(m, seg_end[-1], d, 2, _lib.ARITH_BF16X3))

    def refused(what, m=m, d=d, ends=seg_end, arith=_lib.ARITH_BF16X3, ws_bytes=None, shift=None, alias=None, null=None):
        loss, lse, dq, flag = Out(1, dev), Out(2 * m if m > 0 else 2, dev), Out(max(m, 1) * max(d, 4), dev), Out(1, dev)
        ws = Scratch(max(ws_ok, 1 << 20), dev)
        args = {"seg_end": (C.c_int64 * max(len(ends), 1))(*ends), "q": qd.data_ptr(), "protos": cd.data_ptr(), "inv_phi": ipd.data_ptr(), "labels": ld.data_ptr(),
                "loss": loss.ptr(), "lse": lse.ptr(), "dq": dq.ptr(), "flag": flag.ptr(), "ws": ws.ptr()}
        if shift:
            args[shift] += 4
        if alias:
            args[alias[0]] = args[alias[1]]
        if null:
            args[null] = None
        rc = lib.ssv_proto_nce(m, d, len(ends), args["seg_end"], args["q"], args["protos"], args["inv_phi"], args["labels"], args["loss"], args["lse"], args["dq"], args["flag"],
                               arith, args["ws"], ws.nbytes if ws_bytes is None else ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        assert rc == INVALID, (what, rc)
        assert lib.ssv_last_error().decode().startswith("ssv_proto_nce:"), (what, lib.ssv_last_error())
        assert loss.untouched() and lse.untouched() and dq.untouched() and flag.untouched() and ws.guard_ok(), f"{what}: an output was touched"
        assert bool((ws.buf == 0xA5).all()), f"{what}: the workspace was touched"

    refused("m = 0", m=0)
    refused("m above the limit", m=8193)
    refused("no segment", ends=())
    refused("nine segments", ends=tuple(range(1, 10)))
    refused("an empty first segment", ends=(0, 64))
    refused("seg_end not increasing", ends=(40, 40))
    refused("seg_end decreasing", ends=(40, 24))
    refused("ktot = 2^31", ends=(40, 1 << 31))
    refused("d no multiple of 4", d=30)
    refused("d = 0", d=0)
    refused("d above the limit", d=8196)
    refused("an unknown arithmetic", arith=5)
    refused("a short workspace", ws_bytes=ws_ok - 1)
    for name in ("q", "protos", "inv_phi", "labels", "loss", "lse", "dq", "flag", "ws"):
        refused(f"{name} misaligned", shift=name)
        refused(f"{name} NULL", null=name)
    refused("seg_end NULL", null="seg_end")
    refused("dq aliases q", alias=("dq", "q"))
    refused("lse aliases the workspace", alias=("lse", "ws"))
    refused("loss aliases flag", alias=("loss", "flag"))
    # and the same arguments unchanged are accepted
    got = _call(q, protos, inv_phi, labels, seg_end, "bf16x3", dev)
    assert got["flag"] == 0 and bool(torch.isfinite(got["dq"]).all())


@pytest.mark.parametrize("case", [(70, 128, (7, 33, 600), "plain"), (33, 32, (513,), "plain"), (70, 64, (7, 33, 600), "late")], ids=po.case_id)
def test_the_fused_and_the_unfused_route_agree(dev, case):
    """bf16x3 takes the fused kernel at these widths, f32 the GEMM route: each holds the rule against fp64 (above), so they differ by at most twice its bound"""
    from ssv_amd import ops
    assert ops.proto_nce_route(case[1]) == "fused" or ops.ARITHMETIC != "bf16x3"
    ins, r64, r32 = _refs(case)
    fused, unfused = _call(*ins, "bf16x3", dev), _call(*ins, "f32", dev)
    fails = []
    for k in ("loss", "lse", "dq"):
        e, mx = po.errs(fused[k], unfused[k])
        e32, m32 = po.errs(r32[k], r64[k])
        print(f"{po.case_id(case)}.{k}: fused against unfused e {e:.3g} m {mx:.3g} (ref32 {e32:.3g} {m32:.3g})")
        if not (e <= 2 * (FACTOR * e32 + FLOOR) and mx <= 2 * (FACTOR * m32 + FLOOR)):
            fails.append((k, e, mx, e32, m32))
    assert not fails, fails


def test_a_workspace_of_the_stated_size_serves_every_segmentation(dev):
    """ssv_proto_nce_workspace_bytes knows ktot and segs only: 641 rows as (639, 1, 1) - the longest possible segment - and as (214, 214, 213) - the most slices"""
    for sizes in ((639, 1, 1), (214, 214, 213), (1, 1, 639)):
        for d, arith in ((32, "bf16x3"), (36, "bf16x3"), (32, "f32")):
            q, protos, inv_phi, labels, seg_end = po.make_case((33, d, sizes, "plain"))
            got = _call(q, protos, inv_phi, labels, seg_end, arith, dev)
            ref = po.proto_nce(q, protos, inv_phi, labels, seg_end)
            assert got["flag"] == 0 and po.errs(got["dq"], ref["dq"])[0] < 1e-5 and po.errs(got["lse"], ref["lse"])[0] < 1e-5
