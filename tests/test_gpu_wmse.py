"""GPU: the batched whitening of W-MSE (csrc/whiten.hip: ssv_whiten_fwd / ssv_whiten_bwd / ssv_wmse_perm) straight through the C ABI against tests/wmse_oracle.py
(fp64, torch.linalg under autograd) on the same fp32 inputs - accuracy, buffer hygiene, the contract cases, the refusals, the permutation -; then
utils.losses.WmseLoss against the oracle fed fn.last_perm, the trainer, the step graph and the command line.

Accuracy.  Rules (a) and (d) of tests/test_gpu_loss_kernels.py.  With ref64 = the oracle in float64 on the CPU, ref32 = the same lines in float32,
e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64|, for y, mean, winv and dx of every case of wmse_oracle.CASES x SEEDS x EPSES, for
C = y^T y / (w - 1) against its exact value I at eps = 0, and for the loss, dz1 and dz2 of WmseLoss:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
FLOOR = 2 * 2^-24.  FACTOR is the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured on an MI355X against ref32
(profiles/wmse_kernels_report.json, written by this file under SSV_WMSE_REPORT=<path>), rounded up to the next power of two and never above 8.
The cases keep cond(S) <= 2e4 (tests/test_wmse_cpu.py), so ref32 itself is meaningful.
Measured (210 figures): 1.78 at worst - m of dz1 at 16 x 4, w_size 8, eps 0 in both arithmetics (the whitening runs no GEMM, the two agree bit for bit) - then m
of winv 1.62 and e of dx 1.13 at 2 x 8 x 4, eps 1e-3; everything at 36 columns and wider is below 0.61 (every sum of the kernels runs in double, so at the larger
shapes they are closer to fp64 than the fp32 reference is) - so FACTOR is 2."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wmse_oracle as wo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 1024
FACTOR = 2.0
FLOOR = 2 * U
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
    path = os.environ.get("SSV_WMSE_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """n floats of NaN with GUARD floats of NaN behind them (as int32 the NaN is 0x7fc00000: no status the kernels write)"""

    def __init__(self, n, dev):
        self.n, self.buf = n, torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def t(self):
        return self.buf[:self.n]

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool(torch.isnan(self.buf[self.n:]).all())

    def written(self):
        return not bool(torch.isnan(self.t).any()) and self.guard_ok()

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


class Scratch:
    """the workspace: ``fill`` bytes, with 4 * GUARD bytes of 0xA5 behind them"""

    def __init__(self, blocks, w, d, dev, fill=0xA5):
        from ssv_amd import _lib
        self.nbytes = int(_lib.load().ssv_whiten_workspace_bytes(blocks, w, d))
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[:self.nbytes] = fill

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _fwd(x, rows, eps, dev, fill=0xA5):
    """ssv_whiten_fwd through the C ABI on guarded buffers: x [n_rows, d] fp32 and rows [blocks, w] int32 device tensors -> {y, mean, winv (fp32), info (int32)} on the CPU"""
    from ssv_amd import _lib
    (n_rows, d), (blocks, w) = x.shape, rows.shape
    x0, r0 = x.clone(), rows.clone()
    y, mean, winv, info = Out(blocks * w * d, dev), Out(blocks * d, dev), Out(blocks * d * d, dev), Out(blocks, dev)
    ws = Scratch(blocks, w, d, dev, fill)
    _lib.call("ssv_whiten_fwd", blocks, w, d, n_rows, x.data_ptr(), rows.data_ptr(), float(eps), y.ptr(), mean.ptr(), winv.ptr(), info.ptr(), ws.ptr(), ws.nbytes,
              _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    assert y.guard_ok() and mean.guard_ok() and winv.guard_ok() and info.guard_ok(), "an output guard was written"
    assert torch.equal(_bits(x), _bits(x0)) and torch.equal(rows, r0), "an input was written"
    return {"y": y.t.view(blocks * w, d).cpu(), "mean": mean.t.view(blocks, d).cpu(), "winv": winv.t.view(blocks, d, d).cpu(), "info": info.t.view(torch.int32).cpu()}


def _bwd(x, rows, eps, mean, winv, dy, dev, fill=0xA5):
    """ssv_whiten_bwd on guarded buffers -> dx [n_rows, d] on the CPU, NaN where nothing was written"""
    from ssv_amd import _lib
    (n_rows, d), (blocks, w) = x.shape, rows.shape
    ins = [x, rows, mean, winv, dy]
    before = [t.clone() for t in ins]
    dx = Out(n_rows * d, dev)
    ws = Scratch(blocks, w, d, dev, fill)
    _lib.call("ssv_whiten_bwd", blocks, w, d, n_rows, x.data_ptr(), rows.data_ptr(), float(eps), mean.data_ptr(), winv.data_ptr(), dy.data_ptr(), dx.ptr(), ws.ptr(),
              ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok() and dx.guard_ok(), "a guard was written"
    for a, b in zip(ins, before):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), "an input was written"
    return dx.t.view(n_rows, d).cpu()


# ---- accuracy against fp64 --------------------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _inputs(case, seed):
    blocks, w, d = case
    x, rows = wo.make_case(blocks, w, d, seed), wo.make_rows(blocks, w, seed)
    dy = torch.randn(blocks * w, d, generator=torch.Generator().manual_seed(50 + seed), dtype=torch.float64).to(torch.float32)
    return x, rows, dy


def _refs(case, seed, eps):
    """the fp64 oracle and its fp32 evaluation, computed once per (case, seed, eps) and never modified"""
    key = (case, seed, eps)
    if key not in _REFS:
        x, rows, dy = _inputs(case, seed)
        e32 = float(np.float32(eps))                                      # the fp32 value the kernel receives
        _REFS[key] = (wo.whiten_with_grad(x, rows, e32, dy, torch.float64), wo.whiten_with_grad(x, rows, e32, dy, torch.float32))
    return _REFS[key]


def _figures(got, ref64, ref32):
    e, m = wo.errs(got, ref64)
    e32, m32 = wo.errs(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32, fails):
    f = REPORT[f"{name}.{what}"] = _figures(got.detach().cpu(), ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})  ratios {f['ratio_e']:.3g} {f['ratio_m']:.3g}")
    if not (f["e"] <= FACTOR * f["e_ref32"] + FLOOR and f["m"] <= FACTOR * f["m_ref32"] + FLOOR):
        fails.append((name, what, f))


def _cov(y, blocks, w):
    yb = y.to(torch.float64).view(blocks, w, -1)
    return yb.transpose(1, 2) @ yb / (w - 1)


@pytest.mark.parametrize("eps", wo.EPSES)
@pytest.mark.parametrize("seed", wo.SEEDS)
@pytest.mark.parametrize("case", wo.CASES, ids=lambda c: "x".join(map(str, c)))
def test_whitening_against_fp64(dev, case, seed, eps):
    blocks, w, d = case
    x, rows, dy = _inputs(case, seed)
    r64, r32 = _refs(case, seed, eps)
    xd, rd, dyd = x.to(dev), rows.to(dev), dy.to(dev)
    got = _fwd(xd, rd, eps, dev, 0xA5)
    again = _fwd(xd, rd, eps, dev, 0x00)
    assert bool((got["info"] == 0).all()), got["info"]
    for k in ("y", "mean", "winv"):
        assert not bool(torch.isnan(got[k]).any()), f"{k} was not written everywhere"
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{k} depends on what the workspace held"
    assert bool((torch.triu(got["winv"], diagonal=1) == 0).all()), "winv must carry exact zeros above the diagonal"
    md, wd = got["mean"].to(dev), got["winv"].to(dev)
    dx = _bwd(xd, rd, eps, md, wd, dyd, dev, 0xA5)
    dx2 = _bwd(xd, rd, eps, md, wd, dyd, dev, 0x00)
    assert not bool(torch.isnan(dx).any()) and torch.equal(_bits(dx), _bits(dx2)), "dx is incomplete or depends on what the workspace held"
    tag = f"{blocks}x{w}x{d}-s{seed}-eps{eps:g}"
    fails = []
    for k in ("y", "mean", "winv"):
        _hold(tag, k, got[k], r64[k], r32[k], fails)
    _hold(tag, "dx", dx, r64["dx"], r32["dx"], fails)
    if eps == 0.0:
        eye = torch.eye(d, dtype=torch.float64).expand(blocks, d, d)
        _hold(tag, "cov", _cov(got["y"], blocks, w), eye, _cov(r32["y"], blocks, w), fails)
    assert not fails, fails


# ---- the contract cases -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_non_positive_pivot_is_reported_and_stays_inside_its_block(dev):
    blocks, w, d = 3, 16, 8                                               # w a power of two: the mean of a constant column is exact, its centred column exactly zero
    x = wo.make_case(blocks, w, d, 0)
    rows = torch.arange(blocks * w, dtype=torch.int32).view(blocks, w)
    x[rows[1].long(), 5] = 3.25
    full = _fwd(x.to(dev), rows.to(dev), 0.0, dev)
    assert full["info"].tolist() == [0, 6, 0], full["info"]
    assert bool(torch.isnan(full["y"][w:2 * w]).all()) and bool(torch.isnan(full["winv"][1]).all())
    assert torch.equal(full["mean"][1], x[rows[1].long()].double().mean(dim=0).float())
    rest = _fwd(x.to(dev), rows[[0, 2]].contiguous().to(dev), 0.0, dev)
    assert rest["info"].tolist() == [0, 0]
    for k, a, b in (("y", torch.cat([full["y"][:w], full["y"][2 * w:]]), rest["y"]), ("mean", full["mean"][[0, 2]], rest["mean"]), ("winv", full["winv"][[0, 2]], rest["winv"])):
        assert not bool(torch.isnan(a).any()) and torch.equal(_bits(a), _bits(b)), f"{k} of a good block changed with the bad block beside it"
    # the backward of the call: NaN rows for the failed block, the others as without it
    dy = torch.randn(blocks * w, d, generator=torch.Generator().manual_seed(3))
    dx = _bwd(x.to(dev), rows.to(dev), 0.0, full["mean"].to(dev), full["winv"].to(dev), dy.to(dev), dev)
    assert bool(torch.isnan(dx[rows[1].long()]).all()) and not bool(torch.isnan(dx[rows[[0, 2]].flatten().long()]).any())
    # with eps > 0 the same block factors
    assert _fwd(x.to(dev), rows.to(dev), 1e-3, dev)["info"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("bad", [-1, "n_rows"])
def test_an_index_out_of_range_is_never_dereferenced(dev, bad):
    blocks, w, d, n_rows = 3, 24, 12, 72
    big = torch.full((n_rows + 2, d), float("nan"))                         # x is a window of a larger buffer: row -1 and row n_rows exist and hold NaN
    big[1:n_rows + 1] = wo.make_case(blocks, w, d, 1)
    x = big.to(dev)[1:n_rows + 1]
    assert x.data_ptr() % 16 == 0
    rows = wo.make_rows(blocks, w, 1)
    rows[2, 7] = n_rows if bad == "n_rows" else bad
    out = _fwd(x, rows.to(dev), 1e-3, dev)
    assert out["info"].tolist() == [0, 0, -1]
    assert bool(torch.isnan(out["y"][2 * w:]).all()) and bool(torch.isnan(out["winv"][2]).all()) and bool(torch.isnan(out["mean"][2]).all())
    assert not bool(torch.isnan(out["y"][:2 * w]).any())
    good = _fwd(x, rows[:2].contiguous().to(dev), 1e-3, dev)
    assert torch.equal(_bits(out["y"][:2 * w]), _bits(good["y"])) and torch.equal(_bits(out["winv"][:2]), _bits(good["winv"]))
    mean, winv = out["mean"].clone(), out["winv"].clone()
    mean[2], winv[2] = 0.0, torch.eye(d)
    dx = _bwd(x, rows.to(dev), 1e-3, mean.to(dev), winv.to(dev), torch.ones(blocks * w, d, device=dev), dev)
    named = [r for r in rows[2].tolist() if 0 <= r < n_rows]
    assert bool(torch.isnan(dx[named]).all()) and not bool(torch.isnan(dx[rows[:2].flatten().long()]).any())


def test_rows_no_block_names_are_left_untouched(dev):
    blocks, w, d, n_rows = 2, 24, 12, 100
    x = wo.make_case(5, 20, d, 2)
    assert x.shape[0] == n_rows
    rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:blocks * w].to(torch.int32).view(blocks, w).contiguous()
    f = _fwd(x.to(dev), rows.to(dev), 0.0, dev)
    dy = torch.randn(blocks * w, d, generator=torch.Generator().manual_seed(6))
    dx = _bwd(x.to(dev), rows.to(dev), 0.0, f["mean"].to(dev), f["winv"].to(dev), dy.to(dev), dev)
    named = torch.zeros(n_rows, dtype=torch.bool)
    named[rows.flatten().long()] = True
    assert bool(torch.isnan(dx[~named]).all()), "a row outside `rows` was written"
    assert not bool(torch.isnan(dx[named]).any())
    # the compact oracle: the same blocks of the gathered rows
    ref = wo.whiten_with_grad(x, rows, 0.0, dy)
    assert wo.errs(dx[named], ref["dx"][named])[1] <= 1e-4


def test_a_duplicate_block_gives_identical_bits_at_another_position(dev):
    blocks, w, d = 3, 40, 36
    x = wo.make_case(blocks, w, d, 0)
    rows = wo.make_rows(blocks, w, 0)
    rows4 = torch.cat([rows, rows[:1]]).contiguous()                        # block 3 repeats block 0
    f = _fwd(x.to(dev), rows4.to(dev), 1e-3, dev)
    assert f["info"].tolist() == [0, 0, 0, 0]
    assert torch.equal(_bits(f["y"][:w]), _bits(f["y"][3 * w:])) and torch.equal(_bits(f["mean"][0]), _bits(f["mean"][3])) and torch.equal(_bits(f["winv"][0]), _bits(f["winv"][3]))
    # the backward needs distinct indices: the copy lives in a second copy of x
    x2 = torch.cat([x, x])
    rows4[3] += blocks * w
    dy = torch.randn(blocks * w, d, generator=torch.Generator().manual_seed(8))
    dy4 = torch.cat([dy, dy[:w]])
    f2 = _fwd(x2.to(dev), rows4.to(dev), 1e-3, dev)
    dx = _bwd(x2.to(dev), rows4.to(dev), 1e-3, f2["mean"].to(dev), f2["winv"].to(dev), dy4.to(dev), dev)
    assert torch.equal(_bits(dx[rows4[0].long()]), _bits(dx[rows4[3].long()]))


def test_refusals_leave_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4096 * 132, device=dev)
    rows = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    outs = [Out(1 << 16, dev) for _ in range(5)]
    y, mean, winv, info, dx = outs
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    st = _lib.stream()

    def fwd(blocks=8, w=128, d=64, n_rows=1024, eps=0.0, xp=0, yp=0, wsp=0, ws_bytes=None, rowsp=0):
        return lib.ssv_whiten_fwd(blocks, w, d, n_rows, x.data_ptr() + xp, rows.data_ptr() + rowsp, eps, y.ptr() + yp, mean.ptr(), winv.ptr(), info.ptr(), ws.data_ptr() + wsp,
                                  ws.numel() if ws_bytes is None else ws_bytes, st)

    def bwd(blocks=8, w=128, d=64, n_rows=1024, eps=0.0, dxp=0, ws_bytes=None, dx_ptr=None):
        return lib.ssv_whiten_bwd(blocks, w, d, n_rows, x.data_ptr(), rows.data_ptr(), eps, mean.ptr(), winv.ptr(), y.ptr(), (dx.ptr() if dx_ptr is None else dx_ptr) + dxp,
                                  ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, st)

    need = lib.ssv_whiten_workspace_bytes(8, 128, 64)
    for shape in wo.REFUSED_SHAPES:
        assert fwd(*shape) == INVALID and bwd(*shape) == INVALID, shape
    for kw in ({"eps": 1.0}, {"eps": -1e-3}, {"eps": float("nan")}, {"n_rows": 0}, {"n_rows": 1 << 31}, {"ws_bytes": need - 1}):
        assert fwd(**kw) == INVALID and bwd(**kw) == INVALID, kw
    for kw in ({"xp": 4}, {"yp": 8}, {"wsp": 4}, {"rowsp": 4}):
        assert fwd(**kw) == INVALID, kw
    assert bwd(dxp=4) == INVALID
    assert bwd(dx_ptr=x.data_ptr()) == INVALID, "dx may not alias x"
    assert lib.ssv_whiten_fwd(8, 128, 64, 1024, x.data_ptr(), rows.data_ptr(), 0.0, y.ptr(), y.ptr(), winv.ptr(), info.ptr(), ws.data_ptr(), ws.numel(), st) == INVALID
    assert lib.ssv_whiten_fwd(8, 128, 64, 1024, x.data_ptr(), rows.data_ptr(), 0.0, x.data_ptr(), mean.ptr(), winv.ptr(), info.ptr(), ws.data_ptr(), ws.numel(), st) == INVALID
    perm = Out(4096, dev)
    for n, views, iters in ((1, 1, 1), (4097, 1, 1), (64, 0, 1), (64, 9, 1), (64, 2, 0), (64, 2, 17)):
        assert lib.ssv_wmse_perm(n, views, iters, 0, 0, None, perm.ptr(), st) == INVALID
    assert lib.ssv_wmse_perm(64, 2, 1, 0, 0, None, perm.ptr() + 4, st) == INVALID
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs) and perm.untouched() and not bool(ws.any()) and not bool(x.any())
    assert fwd() == 0                                                     # the same buffers, accepted: x = 0 has no Cholesky factor
    torch.cuda.synchronize()
    assert info.t.view(torch.int32)[:8].tolist() == [1] * 8


# ---- the permutation --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,views,iters,seed,step", [(2, 1, 1, 0, 0), (37, 3, 2, 9, 4), (512, 2, 4, 0, 123456789), (4096, 8, 2, 2 ** 40 + 5, 7), (1030, 2, 16, 1, 2 ** 32 - 1)])
def test_permutation_is_the_argsort_of_the_philox_keys(dev, n, views, iters, seed, step):
    from ssv_amd import ops
    p = ops.wmse_perm(n, views, iters, seed, step=step, device=dev)
    q = ops.wmse_perm(n, views, iters, seed, step=step, device=dev)
    torch.cuda.synchronize()
    assert p.dtype == torch.int32 and tuple(p.shape) == (iters, views, n) and torch.equal(p, q)
    for t in range(iters):
        assert torch.equal(p[t, 0].sort().values.cpu(), torch.arange(n, dtype=torch.int32))
        for v in range(views):
            assert torch.equal(p[t, v], p[t, 0] + v * n)
    want = wo.perm(n, views, min(iters, 2), seed, step)                   # the Python restatement is slow: two iterations say as much as sixteen
    assert torch.equal(p[:want.shape[0]].cpu(), want)


def test_permutation_step_counter_in_device_memory(dev):
    from ssv_amd import ops
    step_dev = torch.full((1,), 41, dtype=torch.int64, device=dev)
    got = [ops.wmse_perm(64, 2, 2, 5, step_dev=step_dev) for _ in range(3)]
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 44
    for k, p in enumerate(got):
        assert torch.equal(p, ops.wmse_perm(64, 2, 2, 5, step=41 + k, device=dev))
    assert not torch.equal(got[0], got[1])


def test_permutation_reaches_every_position(dev):
    """n = 8 over 256 steps: every value at every position.  A sound generator misses one of the 64 (value, position) cells with probability 64 (7/8)^256 < 1e-13."""
    from ssv_amd import ops
    seen = torch.zeros(8, 8, dtype=torch.bool)
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    perms = torch.stack([ops.wmse_perm(8, 1, 1, 0, step_dev=step_dev)[0, 0] for _ in range(256)]).cpu()
    assert int(step_dev.item()) == 256
    for pos in range(8):
        seen[pos, perms[:, pos].long().unique()] = True
    assert bool(seen.all())


# ---- the loss module --------------------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(16, 4, 8, 1), (48, 12, 24, 4), (52, 12, 24, 2), (512, 64, 128, 1)]


def _loss_inputs(n, d):
    g = torch.Generator().manual_seed(11 * n + d)
    base = torch.randn(n, d, generator=g, dtype=torch.float64)
    mix = torch.eye(d, dtype=torch.float64) + 0.3 * torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
    z1 = (base + 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)) @ mix + 1.0
    z2 = (base + 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64)) @ mix + 1.0
    return z1.to(torch.float32), z2.to(torch.float32)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("eps", wo.EPSES)
@pytest.mark.parametrize("n,d,w_size,w_iter", LOSS_SHAPES)
def test_loss_module_against_fp64(dev, n, d, w_size, w_iter, eps, arith):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    c1, c2 = _loss_inputs(n, d)
    z1, z2 = c1.to(dev).requires_grad_(True), c2.to(dev).requires_grad_(True)
    fn = losses.WmseLoss(w_size, w_iter, eps, seed=3)
    with ops.arithmetic(arith):
        loss = fn(z1, z2)
        loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(z1.detach()), _bits(c1.to(dev))) and torch.equal(_bits(z2.detach()), _bits(c2.to(dev))), "an input was written"
    perm = fn.last_perm.cpu()
    assert tuple(perm.shape) == (w_iter, 2, n) and torch.equal(perm, wo.perm(n, 2, w_iter, 3, 0)) and int(fn.step_dev.item()) == 1
    assert len(fn.last_info) == w_iter and all(bool((i == 0).all()) for i in fn.last_info)
    e32 = float(np.float32(eps))
    r64, r32 = wo.wmse_loss(c1, c2, perm, w_size, e32, torch.float64), wo.wmse_loss(c1, c2, perm, w_size, e32, torch.float32)
    assert 0.0 < float(r64[0]) < 4.0
    tag = f"loss-{n}x{d}-w{w_size}-it{w_iter}-eps{eps:g}[{arith}]"
    fails = []
    _hold(tag, "loss", loss.detach().reshape(1), r64[0].reshape(1), r32[0].reshape(1), fails)
    _hold(tag, "dz1", z1.grad, r64[1], r32[1], fails)
    _hold(tag, "dz2", z2.grad, r64[2], r32[2], fails)
    assert not fails, fails
    nb = n // w_size
    if nb * w_size < n:                                                   # ragged: rows no iteration names get exactly zero gradient, in both views
        left = sorted(set(range(n)) - set(perm[:, 0, :nb * w_size].flatten().tolist()))
        if left:
            assert float(z1.grad[left].abs().max()) == 0.0 and float(z2.grad[left].abs().max()) == 0.0
        one = losses.WmseLoss(w_size, 1, eps, seed=4)
        a, b = c1.to(dev).requires_grad_(True), c2.to(dev).requires_grad_(True)
        one(a, b).backward()
        left = sorted(set(range(n)) - set(one.last_perm[0, 0, :nb * w_size].cpu().tolist()))
        assert len(left) == n - nb * w_size
        assert float(a.grad[left].abs().max()) == 0.0 and float(b.grad[left].abs().max()) == 0.0
        used = sorted(set(range(n)) - set(left))
        assert float(a.grad[used].abs().min(dim=1).values.max()) > 0.0


def test_loss_module_check_names_the_block(dev):
    from ssv_amd import _lib
    from ssv_amd.utils import losses
    z = torch.randn(16, 4, generator=torch.Generator().manual_seed(1)).to(dev)
    z[:, 2] = 1.5                                                         # a constant column: no block has a Cholesky factor at eps = 0
    fn = losses.WmseLoss(8)
    with pytest.raises(_lib.SsvError, match="block 0"):
        fn(z, z.clone())
    loss = fn(z, z.clone(), check=False)
    assert bool(torch.isnan(loss)) and int(fn.last_info[0][0]) == 3 and int(fn.step_dev.item()) == 2
    assert bool(torch.isfinite(losses.WmseLoss(8, eps=1e-2)(z, z.clone())))


def test_loss_module_is_single_process(dev, monkeypatch):
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import losses
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    z = torch.zeros(16, 4, device=dev)
    with pytest.raises(NotImplementedError):
        losses.WmseLoss(8)(z, z)


def test_projection_head_takes_a_narrow_embedding(dev):
    """emb_dim 4: the last Linear's data gradient contracts over 4 columns, which the library's kernels take in steps of 16 - the head pads.  Against torch in fp64:
    Linear - BatchNorm (batch statistics) - ReLU - Linear, for the output, dx and every parameter gradient."""
    from ssv_amd.models import heads
    torch.manual_seed(5)
    head = heads.WmseProjectionHead(32, 64, 4).to(dev)
    head.train()
    g = torch.Generator().manual_seed(6)
    x, dy = torch.randn(24, 32, generator=g), torch.randn(24, 4, generator=g)
    xd = x.to(dev).requires_grad_(True)
    y = head(xd)
    (y * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in head.state_dict().items()}
    p = {k: sd[k].clone().requires_grad_(True) for k in ("layer1.0.weight", "layer1.0.bias", "layer1.1.weight", "layer1.1.bias", "layer2.weight", "layer2.bias")}
    xr = x.double().requires_grad_(True)
    h = xr @ p["layer1.0.weight"].T + p["layer1.0.bias"]
    h = (h - h.mean(0)) / (h.var(0, unbiased=False) + 1e-5).sqrt() * p["layer1.1.weight"] + p["layer1.1.bias"]
    ref = torch.relu(h) @ p["layer2.weight"].T + p["layer2.bias"]
    (ref * dy.double()).sum().backward()
    assert wo.errs(y, ref)[1] <= 1e-5 and wo.errs(xd.grad, xr.grad)[1] <= 1e-4
    named = dict(head.named_parameters())
    for k, v in p.items():
        if k == "layer1.0.bias":                                          # BatchNorm removes the bias: its exact gradient is 0, the fp32 one rounding noise
            assert float(named[k].grad.abs().max()) <= 1e-5 * float(p["layer1.0.weight"].grad.abs().max())
        else:
            assert wo.errs(named[k].grad, v.grad)[1] <= 1e-4, k


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
def _wmse_config(tmp_path, batch, num_train, num_test, epochs=1):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "wmse_r18_32_synthetic.yaml")))
    cfg["epochs"], cfg["eval_every"] = epochs, 1
    cfg["emb_dim"], cfg["head_hidden_dim"] = 4, 64
    cfg["loss_fn"] = {"w_size": 8, "w_iter": 1, "eps": 0.0}
    cfg["data"]["batch_size"] = batch
    cfg["data"]["synthetic"] = {"num_train": num_train, "num_test": num_test, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"].update(epochs=2, input_dim=4)
    path = tmp_path / "wmse.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    return path


def test_four_steps_eager_and_replayed(dev, tmp_path):
    """Batch 16, emb_dim 4, w_size 8: the four losses are finite, inside (0, 4) and bit-equal between SSV_STEP_GRAPH=0 and SSV_STEP_GRAPH=1 (fresh child processes:
    the switch is read at import); the device step counter ends at 4 on both paths, and every step drew the permutation of its own step number."""
    path = _wmse_config(tmp_path, 16, 64, 32)
    runs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, SSV_STEP_GRAPH=mode, WANDB_MODE="disabled")
        out = tmp_path / f"steps_{mode}.pt"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wmse_steps_child.py"), str(path), str(out)], cwd=tmp_path, env=env, capture_output=True, text=True,
                             timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + "\n" + res.stderr[-3000:]
        runs[mode] = torch.load(out)
    eager, graph = runs["0"], runs["1"]
    assert eager["graph"]["replays"] == 0 and graph["graph"]["disabled"] is None and graph["graph"]["replays"] >= 2, (eager["graph"], graph["graph"])
    for r in (eager, graph):
        assert r["steps"] == [1, 2, 3, 4]
        assert all(np.isfinite(v) and 0.0 < v < 4.0 for v in r["losses"]), r["losses"]
        for s in range(4):
            assert torch.equal(r["perms"][s], wo.perm(16, 2, 1, 0, s)), f"step {s} did not draw the permutation of its step number"
    assert eager["losses"] == graph["losses"], (eager["losses"], graph["losses"])


def test_checkpoint_round_trips_the_two_modules(dev, tmp_path, monkeypatch):
    from conftest import seeded_randn
    from ssv_amd import main as cli
    path = _wmse_config(tmp_path, 16, 64, 32)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    args = {"config": str(path), "arch": "resnet18", "algo": "wmse", "task": "train", "output": "a", "load": None}
    t = cli.trainer_class("wmse")(args=args)
    loss = t.train_step({"aug_1": seeded_randn(1, 16, 3, 32, 32), "aug_2": seeded_randn(2, 16, 3, 32, 32)})["loss"]
    assert np.isfinite(loss) and 0.0 < loss < 4.0
    assert sorted(t._checkpoint_state()) == ["encoder", "proj_head"]
    assert list(t.proj_head.state_dict())[:2] == ["layer1.0.weight", "layer1.0.bias"] and "layer2.weight" in t.proj_head.state_dict()
    t.save_checkpoint()
    t2 = cli.trainer_class("wmse")(args=dict(args, output="b", load=t.output_dir))
    torch.cuda.synchronize()
    for a, b in ((t.encoder, t2.encoder), (t.proj_head, t2.proj_head)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and len(sa) > 0
        assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_trainer_is_single_process(dev, tmp_path, monkeypatch):
    from conftest import seeded_randn
    from ssv_amd import distributed as hdist, main as cli
    path = _wmse_config(tmp_path, 16, 64, 32)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    t = cli.trainer_class("wmse")(args={"config": str(path), "arch": "resnet18", "algo": "wmse", "task": "train", "output": "a", "load": None})
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError):
        t.loss_fn(torch.zeros(16, 4, device=dev), torch.zeros(16, 4, device=dev))


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_wmse(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    path = _wmse_config(tmp_path, 16, 32, 80)                             # one epoch of two steps
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "wmse", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "wmse" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    1/   1 [loss]" in log and "[VALID] Epoch    1/   1 [accuracy]" in log and (out / "best_model.pt").exists()
    torch.cuda.synchronize()
    assert torch.isfinite(model.optim.arena.data).all()
    assert int(model.loss_fn.step_dev.item()) == 2
    state = torch.load(out / "best_model.pt", map_location="cpu")
    assert sorted(state) == ["encoder", "proj_head"]
