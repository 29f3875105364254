"""GPU: NNCLR's nearest-neighbour lookup (csrc/nnlookup.hip: ssv_nn_lookup) straight through the C ABI against an fp64 search on the same fp32 inputs, in both
arithmetics (bf16x3: the fused kernel; f32: the product in the workspace and a row kernel) - the order rule at planted winners, ties, rows behind n, NaN -, buffer
hygiene and refusals; then utils.losses.NnclrLoss against tests/nnclr_oracle.py, the trainer, the step graph and the command line.

Lookup.  With s64 = Q B^T in float64 and tau_i = 2^-14 |q_i| max_j |b_j| (tests/knn_classify_oracle.py's tolerance: both arithmetics form a score of unit vectors
to a few 2^-24, so two bank rows whose fp64 scores differ by less than tau may legitimately swap): a row whose fp64 margin (best minus second best) is at least
tau_i must carry the fp64 arg-max EXACTLY; a row below it is excused - it must still carry an index whose fp64 score is within tau_i of the best - and at most 1 %
of a case's rows may be excused (tests/test_nnclr_cpu.py holds the cases under that cap without a GPU).  |sim - s64[idx]| <= tau_i; nn is out_scale * bank[idx] bit
for bit.

Loss.  Rules (a) and (d) of tests/test_gpu_loss_kernels.py.  With ref64 = tests/nnclr_oracle.py in float64 on the CPU, ref32 = the same lines in float32,
e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64|, for the loss, dp1 and dp2:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
The oracle takes the neighbour indices from fn.last_idx - the lookup tests above have judged them - so a legitimate near-tie cannot fail the loss test.
FLOOR = 2 * 2^-24.  FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured on an MI355X against ref32
(profiles/nnclr_kernels_report.json, written by this file under SSV_NNCLR_REPORT=<path>), rounded up to the next power of two and never above 8.
Measured (36 figures): 1.59 at worst - m of dp1 at 8 x 32 x 16, T 0.1, in both arithmetics (4.61e-7 where ref32 has 2.15e-7: 256 elements, the
GEMMs' accumulation order against the CPU's); e of dp1 1.35 on fp32 MFMA and 0.63 in bf16x3 at the same case, everything at the larger shapes below 0.81, the loss
itself within FLOOR of fp64 everywhere (ratio 0) - so FACTOR is 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnclr_oracle as no

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 1024
FACTOR = 2.0
FLOOR = 2 * U
REPORT = {}
INVALID = -1                                              # SSV_ERR_INVALID
ARITHS = ("bf16x3", "f32")
SCALES = (1.0, 1.0 / 0.1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_NNCLR_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


class Out:
    """n floats of NaN with GUARD floats of NaN behind them (as int32 the NaN is 0x7fc00000: no index of any bank here)"""

    def __init__(self, n, dev):
        self.n, self.buf = n, torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def t(self):
        return self.buf[:self.n]

    def ptr(self):
        return self.buf.data_ptr()

    def written(self):
        return not bool(torch.isnan(self.t).any()) and bool(torch.isnan(self.buf[self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


class Scratch:
    """the workspace: ``fill`` bytes, with 4 * GUARD bytes of 0xA5 behind them"""

    def __init__(self, m, n, d, arith, dev, fill=0xA5):
        from ssv_amd import _lib
        self.nbytes = int(_lib.load().ssv_nn_lookup_workspace_bytes(m, n, d, _code(arith)))
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[:self.nbytes] = fill

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _lookup(q, bank, n, arith, dev, scale=1.0, fill=0xA5, want_nn=True):
    """ssv_nn_lookup through the C ABI on guarded buffers: q [m, d] and bank [>= n, d] device tensors; returns (nn Out or None, idx int64 numpy, sim float32 numpy)"""
    from ssv_amd import _lib
    m, d = q.shape
    q0, b0 = q.clone(), bank.clone()
    nn, idx, sim = Out(m * d, dev) if want_nn else None, Out(m, dev), Out(m, dev)
    ws = Scratch(m, n, d, arith, dev, fill)
    _lib.call("ssv_nn_lookup", m, n, d, q.data_ptr(), bank.data_ptr(), no.f32(scale), nn.ptr() if want_nn else None, idx.ptr(), sim.ptr(), _code(arith),
              ws.ptr(), ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    assert bool(torch.isnan(idx.buf[m:]).all()) and bool(torch.isnan(sim.buf[m:]).all()), "an output guard was written"
    assert torch.equal(_bits(q), _bits(q0)) and torch.equal(_bits(bank), _bits(b0)), "an input was written"
    i = idx.t.view(torch.int32).cpu().numpy().astype(np.int64)
    assert ((i >= 0) & (i < n)).all(), "an index outside [0, n) (or never written)"
    if want_nn:
        assert bool(torch.isnan(nn.buf[m * d:]).all()), "the guard behind nn was written"
    return nn, i, sim.t.cpu().numpy()


def _gathered(bank, idx, scale):
    """out_scale * bank[idx] as one fp32 multiply per element, on the CPU"""
    return (np.float32(no.f32(scale)) * bank[idx]).astype(np.float32)


# ---- the lookup against fp64 ------------------------------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _case(name, arith, dev):
    """one guarded call per (case, arithmetic, scale), shared by the tests below"""
    if (name, arith) not in _RESULTS:
        q, b = no.lookup_inputs(name)
        c = no.LOOKUP_CASES[name]
        qd, bd = torch.from_numpy(q).to(dev), torch.from_numpy(b).to(dev)
        out = {}
        for scale in SCALES:
            nn, idx, sim = _lookup(qd, bd, c.n, arith, dev, scale)
            assert nn.written()
            out[scale] = (nn.t.view(c.m, c.d).cpu().numpy(), idx, sim)
        _RESULTS[(name, arith)] = out
    return _RESULTS[(name, arith)]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(no.LOOKUP_CASES))
def test_lookup_against_fp64(dev, name, arith):
    r = no.lookup_reference(name)
    _, b = no.lookup_inputs(name)
    rows = np.arange(r["s"].shape[0])
    assert float(r["excused"].mean()) <= no.MAX_EXCUSED
    for scale, (nn, idx, sim) in _case(name, arith, dev).items():
        wrong = idx != r["idx"]
        s_at = r["s"][rows, idx]
        print(f"{name}[{arith}] scale {scale:g}: {int(wrong.sum())} of {len(idx)} rows off the fp64 arg-max ({int(r['excused'].sum())} excused), "
              f"max |sim - s64| {np.abs(sim - s_at).max():.3g} (tau {r['tau'].max():.3g})")
        assert not (wrong & ~r["excused"]).any(), f"rows {np.nonzero(wrong & ~r['excused'])[0][:8]} carry another index than the fp64 arg-max"
        assert (r["best"] - s_at <= r["tau"]).all(), "an excused row's index scores more than tau below the best"
        assert (np.abs(sim.astype(np.float64) - s_at) <= r["tau"]).all()
        assert np.array_equal(nn.view(np.int32), _gathered(b, idx, scale).view(np.int32)), "nn is not out_scale * bank[idx] bit for bit"
    one, ten = _case(name, arith, dev)[SCALES[0]], _case(name, arith, dev)[SCALES[1]]
    assert np.array_equal(one[1], ten[1]) and np.array_equal(one[2].view(np.int32), ten[2].view(np.int32)), "out_scale changed idx or sim"


@pytest.mark.parametrize("name", list(no.LOOKUP_CASES))
def test_both_arithmetics_agree_on_every_row_that_is_not_excused(dev, name):
    r = no.lookup_reference(name)
    a, b = _case(name, "bf16x3", dev)[1.0][1], _case(name, "f32", dev)[1.0][1]
    assert np.array_equal(a[~r["excused"]], b[~r["excused"]])


def _planted(n, d, places, dev, seed, tail=0, tail_fill=0.0):
    """A Gaussian unit-norm bank [n + tail, d] and one query per entry of ``places``: query k is a fresh unit vector planted into the bank at every index of
    places[k] (bit-identical copies).  Rows behind n: ``tail_fill``."""
    g = torch.Generator().manual_seed(seed)
    bank = torch.randn(n + tail, d, generator=g)
    bank = bank / bank.norm(dim=1, keepdim=True)
    q = torch.randn(len(places), d, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    for k, js in enumerate(places):
        for j in js:
            bank[j] = q[k]
    if tail:
        bank[n:] = tail_fill
    return q.to(dev), bank.to(dev)


@pytest.mark.parametrize("arith", ARITHS)
def test_planted_winners_are_found_wherever_they_sit(dev, arith):
    from ssv_amd import ops
    n, d = 1299, 64                                                      # three slices, the last tile ragged
    L = ops.nn_lookup_slice_rows(n)
    assert 128 < L < n - 1
    places = [0, 127, 128, L - 1, L, n - 1]
    q, bank = _planted(n, d, [[j] for j in places], dev, 11)
    _, idx, sim = _lookup(q, bank, n, arith, dev)
    assert idx.tolist() == places
    assert np.abs(sim - 1.0).max() < 1e-5


@pytest.mark.parametrize("arith", ARITHS)
def test_exact_ties_go_to_the_lower_index(dev, arith):
    from ssv_amd import ops
    n, d = 1299, 96
    L = ops.nn_lookup_slice_rows(n)
    pairs = [[3, 17], [40, 200], [5, 36], [100, L + 77], [L - 1, L], [n - 5, n - 2], [64, n - 1], [2 * L + 1, 2 * L + 40, n - 3], [L + 31, L + 32]]
    q, bank = _planted(n, d, pairs, dev, 12)
    _, idx, sim = _lookup(q, bank, n, arith, dev)
    assert idx.tolist() == [p[0] for p in pairs]
    # and bit-identical rows score bit-identically wherever they sit: with the FIRST copy removed the next one wins with the same bits
    bank2 = bank.clone()
    for p in pairs:
        bank2[p[0]] = 0.0
    _, idx2, sim2 = _lookup(q, bank2, n, arith, dev)
    assert idx2.tolist() == [p[1] for p in pairs]
    assert np.array_equal(sim.view(np.int32), sim2.view(np.int32))


@pytest.mark.parametrize("fill", [3.0e30, float("nan")])
@pytest.mark.parametrize("arith", ARITHS)
def test_rows_behind_n_are_never_chosen(dev, arith, fill):
    n, d = 1000, 64                                                      # the last tile is ragged: rows 1000 .. 1015 of the buffer share it
    q, bank = _planted(n, d, [[n - 1], [7]] + [[]] * 30, dev, 13, tail=16, tail_fill=fill)
    clean = bank.clone()
    clean[n:] = 0.0
    nn, idx, sim = _lookup(q, bank, n, arith, dev)
    nn0, idx0, sim0 = _lookup(q, clean, n, arith, dev)
    assert idx[:2].tolist() == [n - 1, 7] and (idx < n).all()
    assert np.array_equal(idx, idx0) and np.array_equal(sim.view(np.int32), sim0.view(np.int32)) and torch.equal(_bits(nn.t), _bits(nn0.t))
    assert nn.written()


@pytest.mark.parametrize("arith", ARITHS)
def test_nan_never_wins(dev, arith):
    n, d = 600, 64
    q, bank = _planted(n, d, [[5], [300], [n - 1]] + [[]] * 5, dev, 14)
    ref = _lookup(q, bank, n, arith, dev)
    # NaN bank rows: the winner of query 0, a row of another tile, the last row.  Their scores are NaN for every query and never chosen
    bank[5] = float("nan")
    bank[130] = float("nan")
    bank[n - 1] = float("nan")
    s = no.scores(q.cpu().numpy(), bank.cpu().numpy())
    want = np.nanargmax(s, axis=1)
    nn, idx, sim = _lookup(q, bank, n, arith, dev)
    assert idx.tolist() == want.tolist() and idx[1] == 300 and not np.isin(idx, (5, 130, n - 1)).any()
    assert not np.isnan(sim).any() and nn.written()
    assert idx[3:].tolist() == ref[1][3:].tolist()
    # an all-NaN query: idx 0, sim -inf, row 0 of the bank; the other queries are what they were
    q2 = q.clone()
    q2[2] = float("nan")
    nn2, idx2, sim2 = _lookup(q2, bank, n, arith, dev, scale=10.0)
    assert idx2[2] == 0 and sim2[2] == -np.inf
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal(idx2[keep], idx[keep]) and np.array_equal(sim2[keep].view(np.int32), sim[keep].view(np.int32))
    assert np.array_equal(nn2.t.view(8, d).cpu().numpy().view(np.int32), _gathered(bank.cpu().numpy(), idx2, 10.0).view(np.int32))


@pytest.mark.parametrize("arith", ARITHS)
def test_buffer_hygiene_and_repeatability(dev, arith):
    name = "130x1000x96-clustered"
    q, b = no.lookup_inputs(name)
    c = no.LOOKUP_CASES[name]
    qd, bd = torch.from_numpy(q).to(dev), torch.from_numpy(b).to(dev)
    runs = [_lookup(qd, bd, c.n, arith, dev, 10.0, fill) for fill in (0xA5, 0xA5, 0x00, 0xFF)]
    for nn, idx, sim in runs:
        assert nn.written() and not np.isnan(sim).any()
    for nn, idx, sim in runs[1:]:                                         # a second call, and workspaces that held other bytes: equal bits
        assert np.array_equal(idx, runs[0][1]) and np.array_equal(sim.view(np.int32), runs[0][2].view(np.int32)) and torch.equal(_bits(nn.t), _bits(runs[0][0].t))
    none, idx, sim = _lookup(qd, bd, c.n, arith, dev, 10.0, want_nn=False)   # nn = NULL is accepted and changes nothing
    assert none is None and np.array_equal(idx, runs[0][1]) and np.array_equal(sim.view(np.int32), runs[0][2].view(np.int32))


def test_ops_wrapper_is_the_entry_point(dev):
    from ssv_amd import _lib, ops
    name = "300x4100x256-gauss"
    q, b = no.lookup_inputs(name)
    c = no.LOOKUP_CASES[name]
    qd = torch.from_numpy(q).to(dev)
    bank = torch.zeros(c.n + 12, c.d, device=dev)
    bank[:c.n] = torch.from_numpy(b).to(dev)
    bank[c.n:] = 50.0
    for arith in ARITHS:
        with ops.arithmetic(arith):
            nn, idx, sim = ops.nn_lookup(qd, bank, n=c.n, out_scale=10.0)
            none, idx2, sim2 = ops.nn_lookup(qd, bank, n=c.n, want_rows=False)
        torch.cuda.synchronize()
        want = _case(name, arith, dev)[SCALES[1]]
        assert idx.dtype == torch.int32 and none is None
        assert np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(idx2.cpu().numpy(), want[1])
        assert np.array_equal(sim.cpu().numpy().view(np.int32), want[2].view(np.int32)) and np.array_equal(nn.cpu().numpy().view(np.int32), want[0].view(np.int32))
    for bad in (lambda: ops.nn_lookup(qd, bank, n=c.n + 13), lambda: ops.nn_lookup(qd, bank, n=0), lambda: ops.nn_lookup(qd[:, :30].contiguous(), bank[:, :30].contiguous()),
                lambda: ops.nn_lookup(qd, bank[:, :64].contiguous()), lambda: ops.nn_lookup(qd, bank, out_scale=float("inf")), lambda: ops.nn_lookup(qd.cpu(), bank)):
        with pytest.raises(_lib.SsvError):
            bad()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    m, n, d = 8, 64, 32
    q, bank = torch.randn(m, d, device=dev), torch.randn(n, d, device=dev)
    for arith in ARITHS:
        nn, idx, sim = Out(m * d, dev), Out(m, dev), Out(m, dev)
        ws = Scratch(m, n, d, arith, dev)
        good = {"m": m, "n": n, "d": d, "q": q.data_ptr(), "bank": bank.data_ptr(), "scale": 1.0, "nn": nn.ptr(), "idx": idx.ptr(), "sim": sim.ptr(), "arith": _code(arith),
                "ws": ws.ptr(), "ws_bytes": ws.nbytes}
        nan, inf = float("nan"), float("inf")
        bad = [{"m": 0}, {"m": -3}, {"m": 8193}, {"n": 0}, {"n": -1}, {"n": 1 << 31}, {"d": 0}, {"d": 30}, {"d": -32}, {"d": 8192 + 4}, {"scale": nan}, {"scale": inf}, {"scale": -inf},
               {"q": None}, {"bank": None}, {"idx": None}, {"sim": None}, {"ws": None},
               {"q": q.data_ptr() + 4}, {"bank": bank.data_ptr() + 8}, {"nn": nn.ptr() + 4}, {"idx": idx.ptr() + 4}, {"sim": sim.ptr() + 8}, {"ws": ws.ptr() + 8},
               {"nn": q.data_ptr()}, {"idx": bank.data_ptr()}, {"sim": idx.ptr()}, {"nn": ws.ptr()},
               {"ws_bytes": ws.nbytes - 1}, {"ws_bytes": 0}, {"arith": 3}, {"arith": -1}]
        order = ("m", "n", "d", "q", "bank", "scale", "nn", "idx", "sim", "arith", "ws", "ws_bytes")
        for change in bad:
            a = dict(good, **change)
            rc = lib.ssv_nn_lookup(*[a[k] for k in order], _lib.stream())
            assert rc == INVALID, (change, rc)
            assert lib.ssv_last_error().decode().startswith("ssv_nn_lookup:"), change
        torch.cuda.synchronize()
        assert nn.untouched() and idx.untouched() and sim.untouched() and bool((ws.buf == 0xA5).all())
        assert lib.ssv_nn_lookup(*[good[k] for k in order], _lib.stream()) == 0                 # and the unchanged arguments are accepted
        torch.cuda.synchronize()
        assert nn.written() and sim.written() and ws.guard_ok()


# ---- the loss module --------------------------------------------------------------------------------------------------------------------------------------------
def _figures(got, ref64, ref32):
    e, m = no.errors(got, ref64)
    e32, m32 = no.errors(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32):
    f = REPORT[f"{name}.{what}"] = _figures(got.detach().cpu(), ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})  ratios {f['ratio_e']:.3g} {f['ratio_m']:.3g}")
    assert f["e"] <= FACTOR * f["e_ref32"] + FLOOR, (name, what, "e", f)
    assert f["m"] <= FACTOR * f["m_ref32"] + FLOOR, (name, what, "m", f)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("temperature", no.TEMPERATURES)
@pytest.mark.parametrize("b,d,n", no.LOSS_SHAPES)
def test_loss_module_against_fp64(dev, b, d, n, temperature, arith):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    cpu = no.loss_inputs(b, d, n)
    z1, z2, p1, p2 = (t.to(dev).requires_grad_(True) for t in cpu[:4])
    bank = cpu[4].to(dev)
    fn = losses.NnclrLoss(temperature)
    with ops.arithmetic(arith):
        loss = fn(z1, z2, p1, p2, bank, n)
        loss.backward()
    torch.cuda.synchronize()
    for got, want in zip((z1, z2, p1, p2, bank), cpu):
        assert torch.equal(_bits(got.detach()), _bits(want.to(dev))), "an input was written"
    assert z1.grad is None and z2.grad is None
    idx = fn.last_idx
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.shape == (2 * b,) and int(idx.min()) >= 0 and int(idx.max()) < n
    # the neighbours are the fp64 arg-max of the normalised projections wherever that is not a near-tie (the lookup's own rule)
    zq = torch.cat(cpu[:2]).double()
    zq = (zq / zq.norm(dim=1, keepdim=True)).float().numpy()
    s = no.scores(zq, cpu[4][:n].numpy())
    two = -np.partition(-s, 1, axis=1)[:, :2]
    clear = two[:, 0] - two[:, 1] >= 4 * no.tau(zq, cpu[4][:n].numpy())      # 4 tau: the GPU normalises in fp32, the queries differ from zq by a few 2^-24
    assert clear.mean() >= 0.95
    assert np.array_equal(idx.cpu().numpy()[clear], s.argmax(1)[clear])
    a = no.neighbours(cpu[4], idx.cpu(), temperature)
    r64, r32 = no.loss_reference(cpu[2], cpu[3], a[:b], a[b:], torch.float64), no.loss_reference(cpu[2], cpu[3], a[:b], a[b:], torch.float32)
    tag = f"{b}x{d}x{n}-T{temperature}[{arith}]"
    _hold(tag, "loss", loss.detach().reshape(1), r64["loss"], r32["loss"])
    _hold(tag, "dp1", p1.grad, r64["dp1"], r32["dp1"])
    _hold(tag, "dp2", p2.grad, r64["dp2"], r32["dp2"])


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("b,d,n", no.LOSS_SHAPES[1:])
def test_loss_module_is_the_composition_spelled_out_here(dev, arith, b, d, n):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    bp = (b + 3) // 4 * 4
    t = 0.1
    cpu = no.loss_inputs(b, d, n)
    bank = cpu[4].to(dev)
    with ops.arithmetic(arith):
        z1, z2, p1, p2 = (x.to(dev).requires_grad_(True) for x in cpu[:4])
        fn = losses.NnclrLoss(t)
        loss = fn(z1, z2, p1, p2, bank, n)
        (3.0 * loss).backward()
        zq = torch.empty(2 * b, d, device=dev)
        ops.l2norm_fwd(cpu[0].to(dev), True, out=zq[:b])
        ops.l2norm_fwd(cpu[1].to(dev), True, out=zq[b:])
        nn, idx, sim = ops.nn_lookup(zq, bank, n=n, out_scale=1.0 / t)
        labels = torch.arange(b, dtype=torch.int32, device=dev)
        stats, grads = [], []
        for a, p in ((nn[:b], cpu[3].to(dev)), (nn[b:], cpu[2].to(dev))):
            phat = torch.zeros(bp, d, device=dev)                         # B rounded up to whole float4s of dlogits; the pad rows are zeros
            _, inv = ops.l2norm_fwd(p, True, out=phat[:b])
            logits = ops.conv2d_fwd(a.view(b, 1, 1, d), phat).view(b, bp)
            st, dlog = ops.softmax_ce(logits, labels, classes=b)
            assert bp == b or bool((dlog[:, b:] == 0).all())
            dphat = torch.empty_like(phat)
            ops.conv2d_wgrad(a.view(b, 1, 1, d), dlog.view(b, 1, 1, bp), phat, dphat, accumulate=False)
            grads.append(ops.l2norm_bwd(phat[:b], inv, dphat[:b], d, True))
            stats.append(st)
        half, three = torch.full((1,), 0.5, device=dev), torch.full((), 3.0, device=dev)
        want = ops.scale_(ops.add_(stats[0][:1], stats[1][:1]), half)
        for g in grads:
            ops.scale_(ops.scale_(g, half), three)
    torch.cuda.synchronize()
    assert torch.equal(fn.last_idx, idx) and torch.equal(_bits(fn.last_sim), _bits(sim))
    assert torch.equal(_bits(loss.detach().reshape(1)), _bits(want))
    assert torch.equal(_bits(p2.grad), _bits(grads[0])) and torch.equal(_bits(p1.grad), _bits(grads[1]))
    assert z1.grad is None and z2.grad is None


def test_loss_module_is_single_process(dev, monkeypatch):
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import losses
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    z = torch.zeros(8, 32, device=dev)
    with pytest.raises(NotImplementedError):
        losses.NnclrLoss()(z, z, z, z, torch.zeros(16, 32, device=dev), 16)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
def _nnclr_config(tmp_path, batch, queue, num_train, num_test, epochs=1):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "nnclr.yaml")))
    cfg["epochs"], cfg["eval_every"] = epochs, 1
    cfg["proj_dim"], cfg["proj_hidden_dim"], cfg["pred_hidden_dim"], cfg["queue_size"] = 64, 128, 128, queue
    cfg["optimizer"]["lr"] = 0.2
    cfg["data"]["batch_size"] = batch
    cfg["data"]["synthetic"] = {"num_train": num_train, "num_test": num_test, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"].update(epochs=2, input_dim=64)
    path = tmp_path / "nnclr.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    return path


def test_four_steps_eager_and_replayed(dev, tmp_path):
    """Batch 32 into a queue of 96 (pad rows: none, 96 = 6 x 16): after every step the device pointer has advanced by 32 modulo 96, the 32 rows just written are
    unit vectors, every other row is bit-unchanged, the loss is finite - and the four losses and the final queue are bit-equal between SSV_STEP_GRAPH=0 and
    SSV_STEP_GRAPH=1 (fresh child processes: the switch is read at import)."""
    from ssv_amd.models.nnclr import seeded_queue
    path = _nnclr_config(tmp_path, 32, 96, 64, 32)
    runs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, SSV_STEP_GRAPH=mode, WANDB_MODE="disabled")
        out = tmp_path / f"steps_{mode}.pt"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nnclr_steps_child.py"), str(path), str(out)], cwd=tmp_path, env=env, capture_output=True, text=True,
                             timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + "\n" + res.stderr[-3000:]
        runs[mode] = torch.load(out)
    eager, graph = runs["0"], runs["1"]
    assert eager["graph"]["replays"] == 0 and graph["graph"]["disabled"] is None and graph["graph"]["replays"] >= 2, (eager["graph"], graph["graph"])
    assert torch.equal(_bits(eager["bank0"]), _bits(seeded_queue(96, 64, 0))), "the queue does not start as the seeded unit-norm rows"
    for r in (eager, graph):
        prev = r["bank0"]
        for s in range(4):
            assert r["ptrs"][s] == (32 * (s + 1)) % 96
            bank = r["banks"][s]
            new = torch.arange(32 * s, 32 * s + 32) % 96
            old = torch.tensor([j for j in range(96) if j not in set(new.tolist())])
            assert float((bank[new].double().norm(dim=1) - 1).abs().max()) <= 1e-6
            assert not torch.equal(bank[new], prev[new])
            assert torch.equal(_bits(bank[old]), _bits(prev[old])), "a queue row outside the 32 just written changed"
            prev = bank
        assert all(np.isfinite(r["losses"]))
    assert eager["losses"] == graph["losses"], (eager["losses"], graph["losses"])
    assert torch.equal(_bits(eager["banks"][-1]), _bits(graph["banks"][-1]))


def test_checkpoint_round_trips_the_three_modules(dev, tmp_path, monkeypatch):
    from conftest import seeded_randn
    from ssv_amd import main as cli
    path = _nnclr_config(tmp_path, 32, 96, 64, 32)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    args = {"config": str(path), "arch": "resnet18", "algo": "nnclr", "task": "train", "output": "a", "load": None}
    t = cli.trainer_class("nnclr")(args=args)
    loss = t.train_step({"aug_1": seeded_randn(1, 32, 3, 32, 32), "aug_2": seeded_randn(2, 32, 3, 32, 32)})["loss"]
    assert np.isfinite(loss)
    assert sorted(t._checkpoint_state()) == ["encoder", "pred_head", "proj_head"]
    assert list(t.proj_head.state_dict())[:2] == ["layer1.0.weight", "layer1.0.bias"] and "layer2.weight" in t.pred_head.state_dict()
    t.save_checkpoint()
    t2 = cli.trainer_class("nnclr")(args=dict(args, output="b", load=t.output_dir))
    torch.cuda.synchronize()
    for a, b in ((t.encoder, t2.encoder), (t.proj_head, t2.proj_head), (t.pred_head, t2.pred_head)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and len(sa) > 0
        assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_nnclr(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    path = _nnclr_config(tmp_path, 16, 48, 32, 80)                        # one epoch of two steps
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "nnclr", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "nnclr" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    1/   1 [loss]" in log and "[VALID] Epoch    1/   1 [accuracy]" in log and (out / "best_model.pt").exists()
    torch.cuda.synchronize()
    assert torch.isfinite(model.optim.arena.data).all()
    assert model.memory_bank.ptr == 32 % 48
    state = torch.load(out / "best_model.pt", map_location="cpu")
    assert sorted(state) == ["encoder", "pred_head", "proj_head"]
