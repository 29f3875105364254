"""GPU: the LARS step (csrc/lars.hip: ssv_lars_step, two launches over the plan of csrc/lars_plan.h) against an fp64 evaluation of the same update on the same
fp32 inputs, straight through the C ABI for every case of tests/lars_oracle.py, then through train_utils.FusedLARS, the step graph and the command line.

Rules (a) and (d) of tests/test_gpu_loss_kernels.py.  With ref64 = tests/lars_oracle.py in float64 on the CPU, ref32 = the same lines in float32,
e(x) = |x - ref64|_2 / |ref64|_2 and m(x) = max|x - ref64| / max|ref64|, for p, mu and the ratio output of every case:
        e(got) <= FACTOR * e(ref32) + FLOOR      and the same for m.
e(ref32) comes from the reference, never from the library (tests/test_lars_cpu.py::test_reference_is_well_conditioned holds it below 1e-3).  FLOOR = 2 * 2^-24:
mu and p are each one fp32 rounding behind their inputs (the resolution of the comparison itself; at most 16 * 2^-24 is allowed).  FACTOR is the worst
max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured on an MI355X against ref32 (profiles/lars_kernels_report.json, written by this file under
SSV_LARS_REPORT=<path>), rounded up to the next power of two and never above 8.  Measured: 0 for every case of the table and for mu and the ratios of the
optimizer test (worst e(got) 4.9e-8 where e(ref32) reaches 3.6e-7), 0.28 for the tensor-by-tensor comparison of the optimizer test (m of a 128-element BatchNorm
tensor after three steps, 1.66e-7: the bits of ref32 itself) - so FACTOR is 1.  The kernels sum the squares in double: the ratio carries one rounding where
ref32's fp32 norms carry several.
(d): p, mu, the ratios and the workspace are views into NaN-prefilled buffers (the workspace: a byte pattern) with 1024 floats of guard behind them; no output
element inside a tensor stays NaN, the guards are untouched, g / g2 / the plan / the four hyper-parameters are bit-identical afterwards.
"""
import json
import os

import numpy as np
import pytest
import torch

import lars_oracle as lo
from conftest import seeded_randn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 1024
FACTOR = 1.0                                              # measured worst ratio 0.28 (see above), rounded up to a power of two
FLOOR = 2 * U
SENTINEL = 0x5EA7BEEF                                     # the bit pattern the padding floats of p and mu carry in the padding test (a finite float)
REPORT = {}
CASES = ["tiny", "chunk_edges", "many", "big", "zero_norms", "no_exclusion", "one_view"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("SSV_LARS_REPORT")
    if path and REPORT:
        from ssv_amd import _lib
        worst = max(max(v["ratio_e"], v["ratio_m"]) for v in REPORT.values())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib.source_sha16(), "factor": FACTOR, "floor": FLOOR, "worst_ratio": worst, "cases": REPORT}, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(n, dev, fill=float("nan")):
    return torch.full((n + GUARD,), fill, dtype=torch.float32, device=dev)


class Arena:
    """The device side of one case: the plan, p / g / g2 / mu laid out as ParamArena does, every buffer with its guard."""

    def __init__(self, lay, tensors, h, dev, two=True, decay=None, adapt=None, gap_p=None, gap_g=None):
        from ssv_amd import _lib
        lib = _lib.load()
        self.lay, self.dev, self.T = lay, dev, len(lay.numels)
        num, off = np.asarray(lay.numels, np.int64), np.asarray(lay.offsets, np.int64)
        dec = np.asarray(lay.decay if decay is None else decay, np.int32)
        ada = np.asarray(lay.adapt if adapt is None else adapt, np.int32)
        self.chunks = int(lib.ssv_lars_plan_chunks(self.T, num.ctypes.data))
        plan = np.zeros(int(lib.ssv_lars_plan_bytes(self.T, num.ctypes.data)), np.uint8)
        _lib.call("ssv_lars_plan_build", self.T, off.ctypes.data, num.ctypes.data, dec.ctypes.data, ada.ctypes.data, plan.ctypes.data, plan.size)
        self.plan = torch.from_numpy(plan).to(dev)
        self.plan0 = self.plan.clone()
        self.hyper = torch.tensor([h["lr"], h["wd"], h["momentum"], h["eta"]], dtype=torch.float32).to(dev)
        self.hyper0 = self.hyper.clone()

        def flat(key, gap):
            host = torch.full((lay.total + GUARD,), float("nan"), dtype=torch.float32)
            if gap is not None:
                host[:lay.total] = gap
            for t, o, n in zip(tensors, lay.offsets, lay.numels):
                host[o:o + n] = t[key].to(torch.float32)
            return host.to(dev)

        self.p, self.mu = flat("p", gap_p), flat("mu", gap_p)
        self.g = flat("g", gap_g)
        self.g2 = flat("g2", gap_g) if (two and tensors[0]["g2"] is not None) else None
        self.before = {k: getattr(self, k).clone() for k in ("p", "mu", "g") + (("g2",) if self.g2 is not None else ())}
        self.ratios = _guarded(self.T, dev)
        self.ws_bytes = int(lib.ssv_lars_workspace_bytes(self.chunks))
        self.ws = torch.full((self.ws_bytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    def step(self):
        from ssv_amd import _lib
        _lib.call("ssv_lars_step", self.lay.total, self.T, self.chunks, self.plan.data_ptr(), self.p.data_ptr(), self.g.data_ptr(), _lib.ptr(self.g2),
                  self.mu.data_ptr(), self.hyper.data_ptr(), self.ratios.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        return self

    def gather(self, flat):
        host = flat.cpu()
        return torch.cat([host[o:o + n] for o, n in zip(self.lay.offsets, self.lay.numels)])

    def gap_mask(self):
        m = torch.ones(self.lay.total + GUARD, dtype=torch.bool)
        for o, n in zip(self.lay.offsets, self.lay.numels):
            m[o:o + n] = False
        return m

    def check_rule_d(self):
        """guards and padding untouched (bit for bit), inputs bit-identical, no NaN left inside a tensor or among the ratios"""
        gaps = self.gap_mask().to(self.dev)
        for k in ("p", "mu"):
            assert torch.equal(_bits(getattr(self, k))[gaps], _bits(self.before[k])[gaps]), f"{k}: a float outside every tensor was written"
            assert torch.isfinite(getattr(self, k)[~gaps]).all(), f"{k}: a non-finite output inside a tensor"
        for k in ("g", "g2"):
            if k in self.before:
                assert torch.equal(_bits(getattr(self, k)), _bits(self.before[k])), f"{k} was written"
        assert torch.equal(self.plan, self.plan0) and torch.equal(_bits(self.hyper), _bits(self.hyper0))
        assert torch.isfinite(self.ratios[:self.T]).all() and torch.isnan(self.ratios[self.T:]).all()
        assert (self.ws[self.ws_bytes:] == 0xA5).all(), "the workspace guard was written"


def _case(name):
    from ssv_amd import _lib
    case = lo.cases(int(_lib.load().ssv_lars_chunk_floats()))[name]
    return case, lo.layout(case), lo.generate(name, case), lo.hyper(case)


def _figures(got, ref64, ref32):
    e, m = lo.errors(got, ref64)
    e32, m32 = lo.errors(ref32, ref64)
    ratio = lambda a, b: 0.0 if a <= FLOOR else (float("inf") if b == 0 else (a - FLOOR) / b)
    return {"e": e, "m": m, "e_ref32": e32, "m_ref32": m32, "ratio_e": ratio(e, e32), "ratio_m": ratio(m, m32)}


def _hold(name, what, got, ref64, ref32):
    f = REPORT[f"{name}.{what}"] = _figures(got, ref64, ref32)
    print(f"{name}.{what}: e {f['e']:.3g} (ref32 {f['e_ref32']:.3g})  m {f['m']:.3g} (ref32 {f['m_ref32']:.3g})")
    assert f["e"] <= FACTOR * f["e_ref32"] + FLOOR, (name, what, "e", f)
    assert f["m"] <= FACTOR * f["m_ref32"] + FLOOR, (name, what, "m", f)


# ---- the kernels against fp64, through the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_step_against_fp64(dev, name):
    case, lay, tensors, h = _case(name)
    a = Arena(lay, tensors, h, dev, two=case.two).step()
    a.check_rule_d()
    ref64, ref32 = lo.reference(name, case, torch.float64), lo.reference(name, case, torch.float32)
    got = (a.gather(a.p), a.gather(a.mu), a.ratios[:a.T].cpu())
    for what, x, r64, r32 in zip(("p", "mu", "q"), got, ref64, ref32):
        _hold(name, what, x, r64, r32)
    q = got[2]
    for t, on in enumerate(lay.adapt):
        if not on:
            assert q[t] == 1.0, (name, t)
    if name == "zero_norms":
        assert q.tolist() == [1.0, 1.0, 1.0]
    if name == "no_exclusion":
        assert all(q[t] != 1.0 for t, s in enumerate(case.shapes) if len(s) <= 1)


# ---- padding ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "chunk_edges", "many"])
def test_padding_is_neither_read_nor_written(dev, name):
    """NaN in the gaps of g and g2 (a gap read into a norm would poison that tensor's ratio), a sentinel bit pattern in the gaps of p and mu."""
    case, lay, tensors, h = _case(name)
    sentinel = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32).item()
    a = Arena(lay, tensors, h, dev, gap_p=sentinel, gap_g=float("nan")).step()
    a.check_rule_d()
    gaps = a.gap_mask()[:lay.total].to(dev)
    assert gaps.any()
    for k in ("p", "mu"):
        assert (_bits(getattr(a, k)[:lay.total])[gaps] == SENTINEL).all()
    plain = Arena(lay, tensors, h, dev).step()                                   # the same bits as with NaN-prefilled gaps: nothing of a gap reaches a tensor
    assert torch.equal(a.gather(a.p), plain.gather(plain.p)) and torch.equal(a.gather(a.mu), plain.gather(plain.mu))
    assert torch.equal(a.ratios[:a.T], plain.ratios[:a.T])


# ---- bitwise identities ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chunk_edges", "big"])
def test_second_identical_call_gives_the_same_bits(dev, name):
    case, lay, tensors, h = _case(name)
    a, b = Arena(lay, tensors, h, dev).step(), Arena(lay, tensors, h, dev).step()
    for k in ("p", "mu", "ratios"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k


@pytest.mark.parametrize("name", ["tiny", "chunk_edges"])
def test_two_slabs_are_the_one_slab_form_on_their_fp32_sum(dev, name):
    case, lay, tensors, h = _case(name)
    summed = [dict(t, g=t["g"] + t["g2"], g2=None) for t in tensors]              # the fp32 sum, rounded once as the kernel rounds it
    a, b = Arena(lay, tensors, h, dev).step(), Arena(lay, summed, h, dev, two=False).step()
    assert a.g2 is not None and b.g2 is None
    for k in ("p", "mu", "ratios"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k


# ---- adapt off everywhere: the formula of plain SGD with momentum -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "chunk_edges"])
def test_without_adaptation_it_is_plain_sgd(dev, name):
    """decay on, adapt off everywhere, one slab, mu = 0: the update of ssv_sgd(nesterov = 0) on a zero buffer.  Within FLOOR, not bitwise: contraction may differ."""
    from ssv_amd import _lib
    case, lay, tensors, h = _case(name)
    T = len(lay.numels)
    one = [dict(t, g=t["g"] + t["g2"], g2=None, mu=torch.zeros_like(t["mu"])) for t in tensors]
    a = Arena(lay, one, h, dev, two=False, decay=[1] * T, adapt=[0] * T, gap_p=0.0, gap_g=0.0).step()
    s = Arena(lay, one, h, dev, two=False, gap_p=0.0, gap_g=0.0)
    _lib.call("ssv_sgd", lay.total, s.p.data_ptr(), s.g.data_ptr(), s.mu.data_ptr(), h["lr"], h["wd"], h["momentum"], 0, 0, _lib.stream())
    torch.cuda.synchronize()
    assert (a.ratios[:T] == 1.0).all()
    for k in ("p", "mu"):
        e, m = lo.errors(a.gather(getattr(a, k)), s.gather(getattr(s, k)).to(torch.float64))
        print(f"{name}.{k} against ssv_sgd: e {e:.3g} m {m:.3g}")
        assert e <= FLOOR and m <= FLOOR, (k, e, m)


# ---- the optimizer ----------------------------------------------------------------------------------------------------------------------------------------------
def _model(dev):
    from ssv_amd.models import heads
    from ssv_amd.networks import resnet
    torch.manual_seed(420)
    enc = resnet.resnet18(reduce_bottom_conv=True).to(dev)
    head = heads.SimclrProjectionHead(512, 128).to(dev)
    return list(enc.parameters()) + list(head.parameters())


@pytest.mark.parametrize("exclude", [True, False])
def test_fused_lars_against_the_oracle_tensor_by_tensor(dev, exclude):
    """ResNet-18 (reduce_bottom_conv) + projector through get_optimizer: seeded gradients written through the p.grad / p._grad_alt views (channels-last filter
    views included), three steps with the learning rate halved before the third; p.data and trust_ratios() against the oracle applied tensor by tensor."""
    from ssv_amd.utils import train_utils
    params = _model(dev)
    cfg = {"name": "lars", "lr": 0.3, "weight_decay": 1e-4, "momentum": 0.9, "eta": 0.001, "exclude_bias_and_norm": exclude}
    opt = train_utils.get_optimizer(cfg, params)
    assert isinstance(opt, train_utils.FusedLARS) and opt.arena.params == params and opt._steps == 0
    assert any(p.dim() == 4 and not p.data.is_contiguous() for p in params), "no channels-last filter view in the arena: the test would not reach them"
    on = [0 if (exclude and p.dim() <= 1) else 1 for p in params]
    state = {dt: [{"p": p.data.detach().cpu().reshape(-1).to(dt), "mu": torch.zeros(p.numel(), dtype=dt)} for p in params] for dt in (torch.float64, torch.float32)}
    q = {}
    for s in range(3):
        if s == 2:
            for g in opt.param_groups:
                g["lr"] *= 0.5
        h = {"lr": lo.f32(opt.param_groups[0]["lr"]), "wd": lo.f32(1e-4), "momentum": lo.f32(0.9), "eta": lo.f32(0.001)}
        opt.zero_grad()
        grads = []
        for i, p in enumerate(params):
            ga, gb = 1e-2 * seeded_randn(1000 * s + 2 * i, *p.shape), 1e-2 * seeded_randn(1000 * s + 2 * i + 1, *p.shape)
            p.grad.copy_(ga.to(dev))
            p._grad_alt.copy_(gb.to(dev))
            grads.append((ga.reshape(-1), gb.reshape(-1)))
        opt.step()
        for dt in state:
            tensors = [dict(t, g=g[0], g2=g[1]) for t, g in zip(state[dt], grads)]
            state[dt], q[dt] = lo.lars_step(tensors, on, on, h, dt)
    torch.cuda.synchronize()
    assert opt._steps == 3
    tag = f"fused.{'exclude' if exclude else 'all'}"
    worst = None
    for i, p in enumerate(params):
        f = _figures(p.data.detach().cpu().reshape(-1), state[torch.float64][i]["p"], state[torch.float32][i]["p"])
        if worst is None or max(f["e"], f["m"]) > max(worst["e"], worst["m"]):
            worst = dict(f, tensor=i, shape=list(p.shape))
        assert f["e"] <= FACTOR * f["e_ref32"] + FLOOR and f["m"] <= FACTOR * f["m_ref32"] + FLOOR, (i, tuple(p.shape), f)
    REPORT[f"{tag}.p_worst_tensor"] = worst
    print(f"{tag}.p, tensor by tensor: worst e {worst['e']:.3g} (ref32 {worst['e_ref32']:.3g}) m {worst['m']:.3g} (ref32 {worst['m_ref32']:.3g}) at tensor {worst['tensor']}")
    mu = torch.cat([opt.momentum_buffer[o:o + p.numel()].cpu() for o, p in zip(opt.arena.offsets, params)])
    # the momentum slab is flat in MEMORY order (OHWI for the filters); norms and element-wise lines do not care, the comparison does: order the oracle's the same way
    order = lambda t, p: t.view(p.shape).permute(0, 2, 3, 1).reshape(-1) if (p.dim() == 4 and not p.data.is_contiguous()) else t
    _hold(tag, "mu", mu, torch.cat([order(t["mu"], p) for t, p in zip(state[torch.float64], params)]),
          torch.cat([order(t["mu"], p) for t, p in zip(state[torch.float32], params)]))
    ratios = opt.trust_ratios().cpu()
    assert ratios.shape == (len(params),)
    _hold(tag, "q", ratios, q[torch.float64], q[torch.float32])
    one_d = [i for i, p in enumerate(params) if p.dim() <= 1]
    assert one_d and len(one_d) < len(params)
    if exclude:
        assert all(ratios[i] == 1.0 for i in one_d)
    else:
        assert all(ratios[i] != 1.0 for i in one_d)
    assert all(0 < ratios[i] < 1 for i in range(len(params)) if i not in one_d)


# ---- the step graph -------------------------------------------------------------------------------------------------------------------------------------------
def _lars_config(tmp_path, batch, num_train, epochs=2):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "simclr.yaml")))
    cfg["epochs"], cfg["eval_every"] = epochs, 1
    cfg["data"]["batch_size"] = batch
    cfg["data"]["synthetic"] = {"num_train": num_train, "num_test": 48, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"]["epochs"] = 2
    cfg["optimizer"] = {"name": "lars", "lr": 0.3, "weight_decay": 1.0e-6, "momentum": 0.9, "eta": 0.001}
    path = tmp_path / "lars.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    return path


def test_replayed_lars_steps_are_bitwise_the_eager_steps(dev, tmp_path, monkeypatch):
    """tests/test_gpu_graph.py::test_replayed_steps_are_bitwise_the_eager_steps with the optimizer block set to LARS: nine steps, the learning rate halved at
    step 5 (four device floats: the same graph)."""
    from ssv_amd import main as cli
    from ssv_amd.graph import StepGraph
    from ssv_amd.utils import train_utils
    path = _lars_config(tmp_path, 64, 128)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    batches = [{"aug_1": seeded_randn(100 + 2 * i, 64, 3, 32, 32).to(dev), "aug_2": seeded_randn(101 + 2 * i, 64, 3, 32, 32).to(dev), "label": torch.zeros(64)} for i in range(9)]
    runs = {}
    for mode in ("eager", "graph"):
        t = cli.trainer_class("simclr")(args={"config": str(path), "arch": "resnet18", "algo": "simclr", "task": "train", "output": mode, "load": None})
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
        runs[mode] = (losses, t.optim.arena.data.clone(), t.optim.momentum_buffer.clone(), t.optim.trust_ratios().clone(), sg.describe(), t.optim._steps)
        sg.close()
    le, pe, me, qe, _, ne = runs["eager"]
    lg, pg, mg, qg, info, ng = runs["graph"]
    assert info["disabled"] is None and info["graphs"] >= 1 and info["replays"] >= 5, info
    assert ne == ng == 9
    assert all(np.isfinite(le)) and le == lg, (le, lg)
    assert torch.equal(pe, pg) and torch.equal(me, mg) and torch.equal(qe, qg)
    assert me.abs().max() > 0


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_simclr_with_lars(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    from ssv_amd.utils import train_utils
    path = _lars_config(tmp_path, 16, 80)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "simclr", "-m", "resnet18", "-t", "train", "-o", "run"])
    assert isinstance(model.optim, train_utils.FusedLARS) and model.optim._steps == 10
    out = tmp_path / "outputs" / "simclr" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    2/   2 [loss]" in log and "[VALID] Epoch    2/   2 [accuracy]" in log and (out / "best_model.pt").exists()
    torch.cuda.synchronize()
    assert torch.isfinite(model.optim.arena.data).all()
    q = model.optim.trust_ratios().cpu()
    assert torch.isfinite(q).all() and (q > 0).all() and (q != 1).any()
