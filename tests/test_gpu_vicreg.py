"""GPU: the VICReg kernels (csrc/vicreg.hip: ssv_vicreg_prep, ssv_vicreg_cgrad) against an fp64 evaluation of the paper's lines on the same fp32 inputs,
straight through the C ABI for every case of tests/vicreg_oracle.py, then through utils.losses.VicregLoss in both arithmetics, the trainer, the step graph and
the command line.

Rules (a) and (d) of tests/test_gpu_loss_kernels.py.  With ref64 = tests/vicreg_oracle.py in float64 on the CPU, ref32 = the same lines in float32,
e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64|, for xc, yc, s, e, parts, G and loss[0:4] of the two entry points and for dx, dy, the
loss and its three terms of VicregLoss:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
e(ref32) comes from the reference, never from the library (tests/test_vicreg_cpu.py::test_reference_is_well_conditioned holds it below 1e-3).  FLOOR = 2 * 2^-24:
the final rounding of an fp32 result, the resolution of the comparison itself (at most 16 * 2^-24 is allowed).  FACTOR is the worst max(0, e(got) - FLOOR) /
e(ref32) (and the same for m) measured on an MI355X against ref32 (profiles/vicreg_kernels_report.json, written by this file under SSV_VICREG_REPORT=<path>),
rounded up to the next power of two and never above 8.
Measured (library source sha16 2456b7add16d385b, 228 figures): 0.45 at worst for the outputs of the two entry points (e of `offset_mean`; xc / yc 0.37, s, parts, G and
loss[0:4] all within FLOOR of fp64: ratio 0) and for the loss and terms of VicregLoss; dx / dy of VicregLoss 2.18 at worst in bf16x3 and 6.75 in f32 (m of dy at
512 x 2048: 1.83e-6 where ref32 has 2.53e-7 - the fp32-MFMA GEMMs' sequential accumulation over 2048 columns against the CPU's blocked one) - so FACTOR is 8.
ssv_vicreg_cgrad is given its own input - the fp64 craw of the case rounded to fp32 and symmetrised, the fp64 parts rounded to fp32 - and held against
vicreg_oracle.cgrad_lines on that input, so its figures are the kernel's, not the GEMM's; the GEMMs are under the bar through VicregLoss.
(d): every output and the workspace are views into NaN-prefilled buffers (the workspace: a byte pattern) with 1024 floats of guard behind them; no output element
stays NaN, the guards are untouched, x and y and parts are bit-identical afterwards.  craw is documented as overwritten (G in place).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lars_oracle as lo
import vicreg_oracle as vo
from conftest import seeded_randn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 1024
FACTOR = 8.0
FLOOR = 2 * U
REPORT = {}
RUNS = vo.runs()
IDS = [r[0] for r in RUNS]
INVALID = -1                                              # SSV_ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_VICREG_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _figures(got, ref64, ref32):
    e, m = vo.errors(got, ref64)
    e32, m32 = vo.errors(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32):
    f = REPORT[f"{name}.{what}"] = _figures(got.detach().cpu(), ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})")
    assert f["e"] <= FACTOR * f["e_ref32"] + FLOOR, (name, what, "e", f)
    assert f["m"] <= FACTOR * f["m_ref32"] + FLOOR, (name, what, "m", f)


class Out:
    """n floats of NaN with GUARD floats of NaN behind them"""

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
    def __init__(self, b, d, dev):
        from ssv_amd import _lib
        self.nbytes = int(_lib.load().ssv_vicreg_workspace_bytes(b, d))
        assert self.nbytes > 0
        self.buf = torch.full((self.nbytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    def ptr(self):
        return self.buf.data_ptr()

    def guard_ok(self):
        return bool((self.buf[self.nbytes:] == 0xA5).all())


def _prep(x, y, coeffs, dev, eps=vo.EPS):
    """ssv_vicreg_prep through the C ABI on guarded buffers; returns the Out objects"""
    from ssv_amd import _lib
    b, d = x.shape
    o = {"xc": Out(2 * b * d, dev), "s": Out(2 * d, dev), "e": Out(2 * b * d, dev), "parts": Out(2, dev)}
    ws = Scratch(b, d, dev)
    _lib.call("ssv_vicreg_prep", b, d, x.data_ptr(), y.data_ptr(), coeffs[0], coeffs[1], coeffs[2], eps,
              o["xc"].ptr(), o["s"].ptr(), o["e"].ptr(), o["parts"].ptr(), ws.ptr(), ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    return o


def _cgrad(craw, b, cov_coeff, parts, dev):
    """ssv_vicreg_cgrad through the C ABI: craw [2, D, D] (CPU) is copied into a guarded buffer and overwritten there; returns (G Out, loss Out)"""
    from ssv_amd import _lib
    d = craw.shape[1]
    g, loss = Out(2 * d * d, dev), Out(4, dev)
    g.t.copy_(craw.reshape(-1))
    ws = Scratch(b, d, dev)
    _lib.call("ssv_vicreg_cgrad", b, d, g.ptr(), cov_coeff, parts.data_ptr(), loss.ptr(), ws.ptr(), ws.nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert ws.guard_ok(), "the workspace guard was written"
    return g, loss


def _cgrad_inputs(run_id, name, coeffs):
    """the fp32 inputs of the direct ssv_vicreg_cgrad call: the case's fp64 craw rounded to fp32 and made exactly symmetric, its fp64 sim and std terms rounded"""
    r64 = vo.reference(run_id, name, coeffs, torch.float64)
    c = r64["craw"].to(torch.float32)
    return ((c + c.transpose(1, 2)) * 0.5).contiguous(), r64["loss"][1:3].to(torch.float32).contiguous()


# ---- the kernels against fp64, through the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_id,name,coeffs", RUNS, ids=IDS)
def test_entry_points_against_fp64(dev, run_id, name, coeffs):
    c = vo.CASES[name]
    b, d = c.B, c.D
    x32, y32 = vo.generate(name)
    x, y = x32.to(dev), y32.to(dev)
    o = _prep(x, y, coeffs, dev)
    for k, v in o.items():
        assert v.written(), f"{k}: a NaN left inside the output, or the guard was written"
    assert torch.equal(_bits(x), _bits(x32.to(dev))) and torch.equal(_bits(y), _bits(y32.to(dev))), "an input was written"
    r64, r32 = vo.reference(run_id, name, coeffs, torch.float64), vo.reference(run_id, name, coeffs, torch.float32)
    _hold(run_id, "xc", o["xc"].t.view(2, b, d)[0], r64["xc"][0], r32["xc"][0])
    _hold(run_id, "yc", o["xc"].t.view(2, b, d)[1], r64["xc"][1], r32["xc"][1])
    _hold(run_id, "s", o["s"].t.view(2, d), r64["s"], r32["s"])
    _hold(run_id, "e", o["e"].t.view(2, b, d), r64["e"], r32["e"])
    _hold(run_id, "parts", o["parts"].t, r64["loss"][1:3], r32["loss"][1:3])

    craw, parts = _cgrad_inputs(run_id, name, coeffs)
    parts_dev = parts.to(dev)
    g, loss = _cgrad(craw, b, coeffs[2], parts_dev, dev)
    assert g.written() and loss.written()
    assert torch.equal(_bits(parts_dev), _bits(parts.to(dev))), "parts was written"
    cov = vo.f32(coeffs[2])
    (g64, l64), (g32, l32) = vo.cgrad_lines(craw, b, cov, parts, torch.float64), vo.cgrad_lines(craw, b, cov, parts, torch.float32)
    _hold(run_id, "G", g.t.view(2, d, d), g64, g32)
    _hold(run_id, "loss", loss.t, l64, l32)
    for i in range(4):                                                      # each of the four scalars on its own as well: a norm over the four hides the small ones
        _hold(run_id, f"loss[{i}]", loss.t[i:i + 1], l64[i:i + 1], l32[i:i + 1])
    gm = g.t.view(2, d, d)
    assert bool((torch.diagonal(gm, dim1=1, dim2=2) == 0).all()), "the diagonal of G is not exactly zero"
    assert torch.equal(_bits(gm), _bits(gm.transpose(1, 2).contiguous())), "G is not its transpose bit for bit where craw was"
    assert torch.equal(_bits(loss.t[1:3]), _bits(parts_dev)), "loss[1:3] is not parts"


# ---- bitwise identities ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["strips", "trips"])
def test_second_identical_call_gives_the_same_bits(dev, name):
    c = vo.CASES[name]
    x, y = (t.to(dev) for t in vo.generate(name))
    a, b_ = _prep(x, y, vo.DEFAULT, dev), _prep(x, y, vo.DEFAULT, dev)
    for k in a:
        assert torch.equal(_bits(a[k].t), _bits(b_[k].t)), k
    craw, parts = _cgrad_inputs(name, name, vo.DEFAULT)
    (g1, l1), (g2, l2) = _cgrad(craw, c.B, 1.0, parts.to(dev), dev), _cgrad(craw, c.B, 1.0, parts.to(dev), dev)
    assert torch.equal(_bits(g1.t), _bits(g2.t)) and torch.equal(_bits(l1.t), _bits(l2.t))


def _sim_term(x32, y32, sim_coeff):
    """g (x - y) and its negation as fp32 lines: g = (float)(2 sim_coeff / (B D)), one subtraction, one multiplication"""
    b, d = x32.shape
    g = torch.tensor(2.0 * vo.f32(sim_coeff) / (float(b) * float(d)), dtype=torch.float32)
    ex = g * (x32 - y32)
    return torch.stack((ex, -ex))


def test_inactive_hinge_leaves_the_sim_term_bit_for_bit(dev):
    x32, y32 = vo.generate("none_active")
    o = _prep(x32.to(dev), y32.to(dev), vo.DEFAULT, dev)
    assert float(o["parts"].t[1]) == 0.0 and float(o["parts"].t[0]) > 0
    assert bool((o["s"].t > 1).all())
    assert torch.equal(_bits(o["e"].t.view(2, *x32.shape).cpu()), _bits(_sim_term(x32, y32, vo.DEFAULT[0])))


def test_a_zero_coefficient_zeroes_its_term_exactly(dev):
    c = vo.CASES["weights"]
    x32, y32 = vo.generate("weights")
    x, y = x32.to(dev), y32.to(dev)
    craw, parts = _cgrad_inputs("weights0", "weights", vo.DEFAULT)
    zero = torch.zeros(2, c.B, c.D)
    # sim alone: no std part in e or parts, G and the cov term zero
    o = _prep(x, y, (1.0, 0.0, 0.0), dev)
    assert float(o["parts"].t[1]) == 0.0 and float(o["parts"].t[0]) > 0
    assert torch.equal(_bits(o["e"].t.view(2, c.B, c.D).cpu()), _bits(_sim_term(x32, y32, 1.0)))
    g, loss = _cgrad(craw, c.B, 0.0, o["parts"].t.clone(), dev)
    assert bool((g.t == 0).all()) and float(loss.t[3]) == 0.0 and float(loss.t[0]) == float(o["parts"].t[0])
    # std alone: no sim part - e is zero wherever the hinge is inactive (the odd columns, scale 4.0)
    o = _prep(x, y, (0.0, 1.0, 0.0), dev)
    e = o["e"].t.view(2, c.B, c.D).cpu()
    assert float(o["parts"].t[0]) == 0.0 and float(o["parts"].t[1]) > 0
    assert torch.equal(e[:, :, 1::2], zero[:, :, 1::2]) and bool((e[:, :, 0::2] != 0).any())
    # cov alone: e and parts zero, the loss is the cov term
    o = _prep(x, y, (0.0, 0.0, 1.0), dev)
    assert torch.equal(o["e"].t.view(2, c.B, c.D).cpu(), zero) and o["parts"].t.tolist() == [0.0, 0.0]
    g, loss = _cgrad(craw, c.B, 1.0, o["parts"].t.clone(), dev)
    assert float(loss.t[3]) > 0 and float(loss.t[0]) == float(loss.t[3]) and loss.t[1:3].tolist() == [0.0, 0.0]


# ---- the loss module ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
@pytest.mark.parametrize("run_id,name,coeffs", RUNS, ids=IDS)
def test_loss_module_against_fp64(dev, run_id, name, coeffs, arith):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    x32, y32 = vo.generate(name)
    x, y = x32.to(dev).requires_grad_(True), y32.to(dev).requires_grad_(True)
    fn = losses.VicregLoss(*coeffs, eps=vo.EPS)
    with ops.arithmetic(arith):
        loss = fn(x, y)
        loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(x.detach()), _bits(x32.to(dev))) and torch.equal(_bits(y.detach()), _bits(y32.to(dev)))
    r64, r32 = vo.reference(run_id, name, coeffs, torch.float64), vo.reference(run_id, name, coeffs, torch.float32)
    tag = f"{run_id}[{arith}]"
    _hold(tag, "loss", loss.detach().reshape(1), r64["loss"][0:1], r32["loss"][0:1])
    _hold(tag, "terms", fn.terms, r64["loss"][1:4], r32["loss"][1:4])
    _hold(tag, "dx", x.grad, r64["dx"], r32["dx"])
    _hold(tag, "dy", y.grad, r64["dy"], r32["dy"])
    assert fn.terms.is_cuda and fn.terms.shape == (3,)


@pytest.mark.parametrize("arith", ["f32", "bf16x3"])
def test_loss_module_is_the_composition_spelled_out_here(dev, arith):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    name = "strips"
    c = vo.CASES[name]
    b, d = c.B, c.D
    x32, y32 = vo.generate(name)
    with ops.arithmetic(arith):
        x, y = x32.to(dev).requires_grad_(True), y32.to(dev).requires_grad_(True)
        fn = losses.VicregLoss()
        loss = fn(x, y)
        (3.0 * loss).backward()
        xc, _, e, parts = ops.vicreg_prep(x32.to(dev), y32.to(dev), 25.0, 25.0, 1.0, 1e-4)
        craw = torch.empty(2, d, d, device=dev)
        for v in range(2):
            ops.conv2d_wgrad(xc[v].view(b, 1, 1, d), xc[v].view(b, 1, 1, d), craw[v], craw[v], accumulate=False)
        loss4, g = ops.vicreg_cgrad(craw, b, 1.0, parts)
        grads = [ops.conv2d_fwd(xc[v].view(b, 1, 1, d), g[v], addend=e[v].view(b, 1, 1, d)).view(b, d) for v in range(2)]
        three = torch.full((), 3.0, device=dev)
        for t in grads:
            ops.scale_(t, three)
    torch.cuda.synchronize()
    assert g.data_ptr() == craw.data_ptr()
    assert torch.equal(_bits(loss.detach().reshape(1)), _bits(loss4[0:1])) and torch.equal(_bits(fn.terms), _bits(loss4[1:4]))
    assert torch.equal(_bits(x.grad), _bits(grads[0])) and torch.equal(_bits(y.grad), _bits(grads[1]))


def test_loss_module_is_single_process(dev, monkeypatch):
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import losses
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    monkeypatch.setattr(hdist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        losses.VicregLoss()(torch.zeros(8, 32, device=dev), torch.zeros(8, 32, device=dev))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dev):
    from ssv_amd import _lib
    lib = _lib.load()
    b, d = 8, 64
    x, y = torch.randn(b, d, device=dev), torch.randn(b, d, device=dev)
    outs = {"xc": Out(2 * b * d, dev), "s": Out(2 * d, dev), "e": Out(2 * b * d, dev), "parts": Out(2, dev)}
    ws = Scratch(b, d, dev)
    good = {"B": b, "D": d, "x": x.data_ptr(), "y": y.data_ptr(), "sim": 25.0, "std": 25.0, "cov": 1.0, "eps": 1e-4, "xc": outs["xc"].ptr(), "s": outs["s"].ptr(),
            "e": outs["e"].ptr(), "parts": outs["parts"].ptr(), "ws": ws.ptr(), "ws_bytes": ws.nbytes}
    nan, inf = float("nan"), float("inf")
    bad = [{"B": 1}, {"B": 0}, {"B": -3}, {"D": 48}, {"D": 0}, {"D": -32}, {"D": 8192 + 32}, {"B": 1 << 20, "D": 8192}, {"sim": -1.0}, {"sim": nan}, {"sim": inf},
           {"std": -1.0}, {"std": nan}, {"std": inf}, {"cov": -1.0}, {"cov": nan}, {"cov": inf}, {"eps": -1e-4}, {"eps": nan}, {"eps": inf},
           {"x": None}, {"y": None}, {"xc": None}, {"s": None}, {"e": None}, {"parts": None}, {"ws": None},
           {"x": x.data_ptr() + 4}, {"y": y.data_ptr() + 8}, {"xc": outs["xc"].ptr() + 4}, {"e": outs["e"].ptr() + 4}, {"ws": ws.ptr() + 8},
           {"ws_bytes": ws.nbytes - 1}, {"ws_bytes": 0}]
    order = ("B", "D", "x", "y", "sim", "std", "cov", "eps", "xc", "s", "e", "parts", "ws", "ws_bytes")
    for change in bad:
        a = dict(good, **change)
        rc = lib.ssv_vicreg_prep(*[a[k] for k in order], _lib.stream())
        assert rc == INVALID, (change, rc)
        assert lib.ssv_last_error().decode().startswith("ssv_vicreg_prep:"), change
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values()) and bool((ws.buf == 0xA5).all())
    assert lib.ssv_vicreg_prep(*[good[k] for k in order], _lib.stream()) == 0              # and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert all(o.written() for o in outs.values())

    craw, loss = Out(2 * d * d, dev), Out(4, dev)
    ws = Scratch(b, d, dev)
    parts = torch.ones(2, device=dev)
    good = {"B": b, "D": d, "craw": craw.ptr(), "cov": 1.0, "parts": parts.data_ptr(), "loss": loss.ptr(), "ws": ws.ptr(), "ws_bytes": ws.nbytes}
    bad = [{"B": 1}, {"B": -3}, {"D": 48}, {"D": 0}, {"D": 8192 + 32}, {"B": 1 << 20, "D": 8192}, {"cov": -1.0}, {"cov": nan}, {"cov": inf},
           {"craw": None}, {"parts": None}, {"loss": None}, {"ws": None}, {"craw": craw.ptr() + 4}, {"ws": ws.ptr() + 8}, {"ws_bytes": ws.nbytes - 1}, {"ws_bytes": 0}]
    order = ("B", "D", "craw", "cov", "parts", "loss", "ws", "ws_bytes")
    for change in bad:
        a = dict(good, **change)
        rc = lib.ssv_vicreg_cgrad(*[a[k] for k in order], _lib.stream())
        assert rc == INVALID, (change, rc)
        assert lib.ssv_last_error().decode().startswith("ssv_vicreg_cgrad:"), change
    torch.cuda.synchronize()
    assert craw.untouched() and loss.untouched() and bool((ws.buf == 0xA5).all()) and parts.tolist() == [1.0, 1.0]


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
# lr 1.0: the scheduler seeds a tenth of it and eta is 1e-3, so a step moves a tensor by ~1e-4 of its norm - visible in fp32 weights
LARS = {"name": "lars", "lr": 1.0, "weight_decay": 1.0e-6, "momentum": 0.9, "eta": 0.001}


def _bare(cls, dev, config):
    from ssv_amd.utils import train_utils
    t = object.__new__(cls)
    t.config, t.device, t.train_loader = config, dev, [None]
    torch.manual_seed(420)
    t._build("resnet18")
    t.scheduler, t.warmup_epochs = train_utils.get_scheduler({**config["scheduler"], "epochs": config["epochs"]}, optimizer=t.optim)
    return t


class _Fp64Model:
    """The same step in plain torch, float64, on the CPU: the oracle's ResNet-18 lines, the projector without a final normalisation, the oracle loss, and
    tests/lars_oracle.py's update tensor by tensor (1-D tensors neither decayed nor adapted, as FusedLARS excludes them by default)."""

    def __init__(self, trainer):
        cast = lambda sd: {k: (v.detach().cpu().double().contiguous().clone() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in sd.items()}
        self.enc, self.head = cast(trainer.encoder.state_dict()), cast(trainer.proj_head.state_dict())
        self.params = [(d, k) for d in (self.enc, self.head) for k in d if k.endswith(".weight") or k.endswith(".bias")]
        for d, k in self.params:
            d[k].requires_grad_(True)
        self.mu = [torch.zeros(d[k].numel(), dtype=torch.float64) for d, k in self.params]

    def embed(self, img):
        from oracle import nets
        p = self.head
        x = nets.resnet_forward(self.enc, img.double(), "resnet18", True)
        x = F.relu(nets._bn_train(F.linear(x, p["layer1.0.weight"], p["layer1.0.bias"]), p, "layer1.1"))
        x = F.relu(nets._bn_train(F.linear(x, p["layer2.0.weight"], p["layer2.0.bias"]), p, "layer2.1"))
        return F.linear(x, p["layer3.weight"], p["layer3.bias"])

    def train_step(self, a1, a2, lr, cfg, loss_cfg):
        loss = vo.loss_lines(self.embed(a1), self.embed(a2), *(vo.f32(loss_cfg[k]) for k in ("sim_coeff", "std_coeff", "cov_coeff", "eps")))[0]
        loss.backward()
        with torch.no_grad():
            for i, (d, k) in enumerate(self.params):
                p = d[k]
                on = p.dim() > 1
                pn, mu, _ = lo.lars_tensor(p.reshape(-1), p.grad.reshape(-1), None, self.mu[i], on, on, lo.f32(lr), lo.f32(cfg["weight_decay"]),
                                           lo.f32(cfg["momentum"]), lo.f32(cfg["eta"]), torch.float64)
                p.copy_(pn.view_as(p))
                self.mu[i] = mu
                p.grad = None
        return float(loss.detach())


def test_first_steps_match_the_fp64_model(dev):
    """Three steps at batch 32 on ResNet-18 (32 x 32), projector width 64.  The bound is the one tests/test_gpu_step.py holds the Barlow Twins steps of the same
    network to: 2e-5 relative on the loss of the first step (one forward: rounding only), 2e-2 on the steps behind an update (two fp32-class evaluations of a
    chaotic trajectory agree in size class only).  The CHANGE of the projector's last-layer weights over the three steps (w3 - w0, which a missing or
    sign-flipped update cannot pass) sits behind the same updates: 2e-2 in relative L2 of the fp64 model's change."""
    from ssv_amd.models.vicreg import VICReg
    loss_cfg = {"sim_coeff": 25.0, "std_coeff": 25.0, "cov_coeff": 1.0, "eps": 1e-4}
    cfg = {"epochs": 1000, "proj_dim": 64, "encoder": {"reduce_bottom_conv": True}, "optimizer": dict(LARS), "scheduler": {"name": "cosine", "warmup_epochs": 10},
           "loss_fn": loss_cfg}
    t = _bare(VICReg, dev, cfg)
    assert sorted(t._checkpoint_state()) == ["encoder", "proj_head"]
    m = _Fp64Model(t)
    w0 = m.head["layer3.weight"].detach().clone()
    got, want = [], []
    for s in range(3):
        a1, a2 = seeded_randn(1400 + 2 * s, 32, 3, 32, 32), seeded_randn(1401 + 2 * s, 32, 3, 32, 32)
        lr = t.optim.param_groups[0]["lr"]
        got.append(t.train_step({"aug_1": a1, "aug_2": a2})["loss"])
        want.append(m.train_step(a1, a2, lr, LARS, loss_cfg))
        print(f"step {s}: loss {got[-1]:.8g} fp64 {want[-1]:.8g} rel {abs(got[-1] - want[-1]) / abs(want[-1]):.3g}")
    torch.cuda.synchronize()
    np.testing.assert_allclose(got[0], want[0], rtol=2e-5)
    np.testing.assert_allclose(got[1:], want[1:], rtol=2e-2)
    # the CHANGE of the weights from the loaded initial state, not the weights: the three LARS updates move a tensor by a few 1e-4 of its norm, so a comparison of the
    # weights themselves would pass without any update at all
    w, w64 = t.proj_head.state_dict()["layer3.weight"].detach().cpu().double(), m.head["layer3.weight"].detach()
    dw, dw64 = w - w0, w64 - w0
    moved = float(dw64.norm() / w0.norm())
    rel = float((dw - dw64).norm() / dw64.norm())
    print(f"layer3.weight after three steps: moved {moved:.3g} of its norm, relative L2 of the change {rel:.3g}")
    assert moved > 1e-6, "the fp64 model's weights did not move: the comparison would measure nothing"
    assert rel < 2e-2
    assert t.loss_fn.terms is not None and bool(torch.isfinite(t.loss_fn.terms).all())


def _vicreg_config(tmp_path, batch, num_train, num_test, epochs=2):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "vicreg.yaml")))
    cfg["epochs"], cfg["eval_every"] = epochs, 1
    cfg["data"]["batch_size"] = batch
    cfg["data"]["synthetic"] = {"num_train": num_train, "num_test": num_test, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"]["epochs"] = 2
    path = tmp_path / "vicreg.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    return path


def test_replayed_steps_are_bitwise_the_eager_steps(dev, tmp_path, monkeypatch):
    """tests/test_gpu_lars.py::test_replayed_lars_steps_are_bitwise_the_eager_steps on the VICReg trainer: nine steps, the learning rate halved at step 5."""
    from ssv_amd import main as cli
    from ssv_amd.graph import StepGraph
    from ssv_amd.utils import train_utils
    path = _vicreg_config(tmp_path, 64, 128, 48)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    batches = [{"aug_1": seeded_randn(100 + 2 * i, 64, 3, 32, 32).to(dev), "aug_2": seeded_randn(101 + 2 * i, 64, 3, 32, 32).to(dev), "label": torch.zeros(64)} for i in range(9)]
    runs = {}
    for mode in ("eager", "graph"):
        t = cli.trainer_class("vicreg")(args={"config": str(path), "arch": "resnet18", "algo": "vicreg", "task": "train", "output": mode, "load": None})
        assert isinstance(t.optim, train_utils.FusedLARS)
        sg = StepGraph(t, mode="1" if mode == "graph" else "0", graph_floors=False)
        losses = []
        for i, batch in enumerate(batches):
            if i == 5:
                for g in t.optim.param_groups:
                    g["lr"] *= 0.5
            losses.append(sg(batch)["loss"])
            t._after_step(i)
        torch.cuda.synchronize()
        runs[mode] = (losses, t.optim.arena.data.clone(), t.optim.momentum_buffer.clone(), sg.describe(), t.optim._steps)
        sg.close()
    le, pe, me, _, ne = runs["eager"]
    lg, pg, mg, info, ng = runs["graph"]
    assert info["disabled"] is None and info["graphs"] >= 1 and info["replays"] >= 5, info
    assert ne == ng == 9
    assert all(np.isfinite(le)) and le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(me, mg)
    assert me.abs().max() > 0


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_vicreg_and_writes_features(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    path = _vicreg_config(tmp_path, 16, 16, 80)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "vicreg", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "vicreg" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    2/   2 [loss]" in log and "[VALID] Epoch    2/   2 [accuracy]" in log and (out / "best_model.pt").exists()
    torch.cuda.synchronize()
    assert torch.isfinite(model.optim.arena.data).all()
    state = torch.load(out / "best_model.pt", map_location="cpu")
    assert list(state["proj_head"])[0] == "layer1.0.weight" and "encoder" in state
    feats = cli.main(["-c", str(path), "-a", "vicreg", "-m", "resnet18", "-t", "get_features", "-o", "feats", "-l", str(out)])
    for split, n in (("train", 16), ("test", 80)):
        f = np.load(os.path.join(feats.output_dir, f"{split}_fvecs.npy"))
        assert f.shape[0] == n and np.isfinite(f).all()
