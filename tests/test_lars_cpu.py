"""CPU: the LARS oracle (tests/lars_oracle.py) against torch.optim.SGD, the conditioning of the case table the GPU tests run (tests/test_gpu_lars.py), the plan
builder of csrc/lars_plan.h through the C ABI and - as a stand-alone program under ASan + UBSan - on its own, and get_optimizer's refusal of bad LARS settings.
No GPU: the plan builder is a pure host function, and the refusals happen before anything touches the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import lars_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND = 1e-3                                              # rule (b) of tests/test_gpu_loss_kernels.py
INVALID, WORKSPACE = -1, -2


def _lib():
    from ssv_amd import _lib
    return _lib


def _c():
    return int(_lib().load().ssv_lars_chunk_floats())


# ---- the oracle against an independent reference ------------------------------------------------------------------------------------------------------------
def _sgd_run(tensors, feed, lr, wd, momentum, steps=3):
    """torch.optim.SGD(momentum, weight_decay, nesterov=False) in fp64 over the same tensors; feed(params, step) -> the gradients of that step."""
    params = [t["p"].to(torch.float64).clone().requires_grad_(True) for t in tensors]
    opt = torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=wd, nesterov=False)
    for s in range(steps):
        for p, gr in zip(params, feed(params, s)):
            p.grad = gr
        opt.step()
    return [p.detach() for p in params]


@pytest.mark.parametrize("adapt", [False, True])
def test_oracle_is_sgd_with_momentum_on_the_scaled_gradient(adapt):
    """adapt off everywhere: three fp64 steps ARE torch.optim.SGD(momentum, weight_decay, nesterov=False) - mu starting at zero makes its first step SGD's
    buffer seeding.  adapt on: they are that SGD with weight_decay 0 fed q_t * u, q_t and u worked out here from the definition."""
    case = lo.cases(_c())["tiny"]
    h = lo.hyper(case)
    T = len(case.shapes)
    tensors = [dict(t, mu=torch.zeros_like(t["mu"])) for t in lo.generate("tiny", case)]
    grads = [[(1 + 0.25 * s) * t["g"].to(torch.float64) + t["g2"].to(torch.float64) for t in tensors] for s in range(3)]     # another gradient every step
    decay = [1, 0, 1, 1]
    state = [dict(t) for t in tensors]
    for s in range(3):
        state = [dict(t, g=grads[s][i], g2=None) for i, t in enumerate(state)]
        state, _ = lo.lars_step(state, decay, [int(adapt)] * T, h, torch.float64)

    def feed_plain(params, s):
        return [grads[s][i] + (0.0 if decay[i] else -h["wd"]) * params[i].detach() for i in range(T)]     # SGD decays everything: take it back where decay is off

    def feed_scaled(params, s):
        out = []
        for i in range(T):
            p = params[i].detach()
            u = grads[s][i] + (h["wd"] if decay[i] else 0.0) * p
            out.append(h["eta"] * p.norm() / u.norm() * u)
        return out

    want = _sgd_run(tensors, feed_scaled, h["lr"], 0.0, h["momentum"]) if adapt else _sgd_run(tensors, feed_plain, h["lr"], h["wd"], h["momentum"])
    for t, w in zip(state, want):
        torch.testing.assert_close(t["p"], w, rtol=1e-12, atol=1e-15)


def test_oracle_ratio_branches():
    case = lo.cases(_c())["zero_norms"]
    lay = lo.layout(case)
    _, q = lo.lars_step(lo.generate("zero_norms", case), lay.decay, lay.adapt, lo.hyper(case), torch.float64)
    assert q.tolist() == [1.0, 1.0, 1.0]
    case = lo.cases(_c())["tiny"]
    lay = lo.layout(case)
    assert lay.adapt == [0, 1, 0, 1] and lay.decay == lay.adapt and lay.offsets == [0, 64, 128, 192] and lay.total == 256
    _, q = lo.lars_step(lo.generate("tiny", case), lay.decay, lay.adapt, lo.hyper(case), torch.float64)
    assert q[0] == 1 and q[2] == 1 and 0 < q[1] < 1 and 0 < q[3] < 1
    nolay = lo.layout(lo.cases(_c())["no_exclusion"])
    assert all(nolay.adapt) and all(nolay.decay)


# ---- conditioning: a condition on the inputs, not a measurement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "chunk_edges", "many", "big", "zero_norms", "no_exclusion", "one_view"])
def test_reference_is_well_conditioned(name):
    case = lo.cases(_c())[name]
    ref64, ref32 = lo.reference(name, case, torch.float64), lo.reference(name, case, torch.float32)
    for what, r64, r32 in zip(("p", "mu", "q"), ref64, ref32):
        assert torch.isfinite(r64).all()
        e, m = lo.errors(r32, r64)
        print(f"{name}.{what}: e(ref32) {e:.3g} m(ref32) {m:.3g}")
        assert e <= COND and m <= COND, (name, what, e, m)


def test_case_table_reaches_what_it_claims():
    c = _c()
    cs = lo.cases(c)
    assert set(cs) == {"tiny", "chunk_edges", "many", "big", "zero_norms", "no_exclusion", "one_view"}
    assert c % 4 == 0 and c >= 256
    numels = lo.layout(cs["chunk_edges"]).numels
    assert numels == [c, c + 1, 2 * c - 1, 3 * c, 64, 5120, 10]
    many = lo.layout(cs["many"])
    assert len(many.numels) == 200 and sorted(set(many.numels)) == [1, 63, 64, 65, 1000] and 0 < sum(many.adapt) < 200
    assert {n for n, a in zip(many.numels, many.adapt) if a} == {n for n, a in zip(many.numels, many.adapt) if not a} == {1, 63, 64, 65, 1000}
    assert min(-(-n // c) for n, a in zip(lo.layout(cs["big"]).numels, lo.layout(cs["big"]).adapt) if a) >= 200        # hundreds of partials per adapted tensor
    assert cs["one_view"].two is False and cs["no_exclusion"].exclude is False


# ---- the plan builder through the C ABI -----------------------------------------------------------------------------------------------------------------------
def _build(offsets, numels, flags, short=0, T=None):
    lib = _lib().load()
    T = len(numels) if T is None else T
    off, num, fl = np.asarray(offsets, np.int64), np.asarray(numels, np.int64), np.asarray(flags, np.int32)
    nbytes, chunks = int(lib.ssv_lars_plan_bytes(T, num.ctypes.data)), int(lib.ssv_lars_plan_chunks(T, num.ctypes.data))
    plan = np.full(max(nbytes - short, 1) + 64, 0xA5, np.uint8)                  # 64 guard bytes behind the buffer
    rc = lib.ssv_lars_plan_build(T, off.ctypes.data, num.ctypes.data, fl.ctypes.data, fl.ctypes.data, plan.ctypes.data, max(nbytes - short, 0))
    assert (plan[max(nbytes - short, 1):] == 0xA5).all(), "the builder wrote behind its buffer"
    if rc != 0:
        return rc, None, None
    ct = plan[:16 * chunks].view(np.dtype([("start", np.int64), ("len", np.int32), ("tensor", np.int32)]))
    tt = plan[16 * chunks:16 * chunks + 16 * T].view(np.dtype([("first", np.int32), ("count", np.int32), ("flags", np.int32), ("reserved", np.int32)]))
    return rc, ct, tt


@pytest.mark.parametrize("name", ["tiny", "chunk_edges", "many", "big", "no_exclusion"])
def test_plan_tiles_every_tensor_exactly_once(name):
    c = _c()
    lay = lo.layout(lo.cases(c)[name])
    rc, ct, tt = _build(lay.offsets, lay.numels, lay.adapt)
    assert rc == 0
    assert (ct["len"] >= 1).all() and (ct["len"] <= c).all()                                            # no chunk is longer than c
    assert tt["first"].tolist() == np.concatenate([[0], np.cumsum(tt["count"])[:-1]]).tolist()           # contiguous, ascending chunk ranges
    assert int(tt["count"].sum()) == len(ct) and (tt["count"] >= 1).all()
    assert tt["flags"].tolist() == [3 if a else 0 for a in lay.adapt]
    for t, (off, n) in enumerate(zip(lay.offsets, lay.numels)):
        mine = ct[tt["first"][t]:tt["first"][t] + tt["count"][t]]
        assert (mine["tensor"] == t).all()
        assert mine["start"].tolist() == [off + k * c for k in range(len(mine))]                        # in order, back to back from the tensor's first float
        assert int(mine["len"].sum()) == n and (mine["len"][:-1] == c).all()                            # ... to its last: tiled once, no chunk across a tensor
    assert (ct["tensor"] == np.repeat(np.arange(len(lay.numels)), tt["count"])).all()


def test_plan_flags_are_independent():
    lib = _lib().load()
    num, off = np.asarray([5, 9], np.int64), np.asarray([0, 64], np.int64)
    decay, adapt = np.asarray([1, 0], np.int32), np.asarray([0, 7], np.int32)
    plan = np.zeros(int(lib.ssv_lars_plan_bytes(2, num.ctypes.data)), np.uint8)
    assert lib.ssv_lars_plan_build(2, off.ctypes.data, num.ctypes.data, decay.ctypes.data, adapt.ctypes.data, plan.ctypes.data, plan.size) == 0
    assert plan[32:].view(np.int32).reshape(2, 4)[:, 2].tolist() == [1, 2]


MALFORMED = {
    "T_zero": dict(offsets=[0], numels=[4], T=0),
    "T_negative": dict(offsets=[0], numels=[4], T=-1),
    "offsets_descend": dict(offsets=[64, 0], numels=[4, 4]),
    "offsets_equal": dict(offsets=[0, 0], numels=[4, 4]),
    "overlap": dict(offsets=[0, 64], numels=[65, 4]),
    "offset_not_multiple_of_4": dict(offsets=[0, 66], numels=[4, 4]),
    "offset_negative": dict(offsets=[-64, 0], numels=[4, 4]),
    "numel_zero": dict(offsets=[0, 64], numels=[4, 0]),
    "numel_negative": dict(offsets=[0, 64], numels=[-4, 4]),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_plan_refuses_malformed_input(name):
    spec = MALFORMED[name]
    lib = _lib().load()
    lib.ssv_lars_plan_build(1, 0, 0, 0, 0, 0, 0)                                  # leaves ANOTHER message behind
    num, off = np.asarray(spec["numels"], np.int64), np.asarray(spec["offsets"], np.int64)
    fl = np.ones(len(num), np.int32)
    T = spec.get("T", len(num))
    plan = np.full(4096, 0xA5, np.uint8)
    rc = lib.ssv_lars_plan_build(T, off.ctypes.data, num.ctypes.data, fl.ctypes.data, fl.ctypes.data, plan.ctypes.data, plan.size)
    assert rc == INVALID and (plan == 0xA5).all()
    msg = lib.ssv_last_error().decode()
    assert msg.startswith("ssv_lars_plan_build: lars plan:") and "null pointer" not in msg, msg


def test_plan_refuses_a_short_buffer_and_null_pointers():
    lib = _lib().load()
    c = _c()
    rc, _, _ = _build([0, c + 64], [c + 1, 5], [1, 1], short=1)
    assert rc == WORKSPACE and "buffer" in lib.ssv_last_error().decode()
    rc, ct, _ = _build([0, c + 64], [c + 1, 5], [1, 1])
    assert rc == 0 and len(ct) == 3
    num = np.asarray([4], np.int64)
    assert lib.ssv_lars_plan_bytes(1, num.ctypes.data) == 32 and lib.ssv_lars_plan_chunks(1, num.ctypes.data) == 1
    assert lib.ssv_lars_plan_bytes(1, None) == 0 and lib.ssv_lars_plan_bytes(0, num.ctypes.data) == 0 and lib.ssv_lars_plan_chunks(1, None) == 0
    assert lib.ssv_lars_workspace_bytes(0) == 0 and lib.ssv_lars_workspace_bytes(3) == 48
    assert lib.ssv_lars_plan_build(1, None, None, None, None, None, 0) == INVALID


# ---- the same plans in a stand-alone program under ASan + UBSan -------------------------------------------------------------------------------------------------
def test_plan_builder_is_clean_under_asan_ubsan(tmp_path):
    """tests/lars_plan_main.cpp + csrc/lars_plan.h compiled as a host program with -fsanitize=address,undefined: every plan of the case table, built into a heap
    buffer of exactly the size the helper names, and every malformed input above.  Exit 0 and no report."""
    cxx = next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/usr/bin/clang++", "/usr/bin/g++") if os.path.exists(p)), "c++")
    exe = tmp_path / "lars_plan_main"
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                          os.path.join(ROOT, "tests", "lars_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    c = _c()
    lines = []
    for name, case in lo.cases(c).items():
        lay = lo.layout(case)
        lines.append(" ".join(map(str, [len(lay.numels), 0] + lay.offsets + lay.numels + lay.adapt)))
        lines.append(" ".join(map(str, [len(lay.numels), "short"] + lay.offsets + lay.numels + lay.adapt)))
    for spec in MALFORMED.values():
        T = spec.get("T", len(spec["numels"]))
        k = max(T, 0)
        lines.append(" ".join(map(str, [T, INVALID] + spec["offsets"][:k] + spec["numels"][:k] + [1] * k)))
    plans = tmp_path / "plans.txt"
    plans.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    run = subprocess.run([str(exe), str(plans)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr, run.stderr[-4000:]
    assert f"{len(lo.cases(c))} built and checked, {len(lo.cases(c)) + len(MALFORMED)} refused" in run.stdout, run.stdout


# ---- configuration ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [{"eta": 0.0}, {"eta": -1e-3}, {"momentum": 1.0}, {"momentum": -0.1}, {"lr": -0.1}, {"weight_decay": -1e-6}])
def test_get_optimizer_refuses_bad_lars_settings_before_the_device(bad):
    from ssv_amd.utils import train_utils
    cfg = dict({"name": "lars", "lr": 0.6, "weight_decay": 1e-6, "momentum": 0.9, "eta": 0.001}, **bad)
    params = [torch.nn.Parameter(torch.zeros(4, 4))]                              # CPU parameters: a device-side refusal would be an SsvError, not this
    with pytest.raises(ValueError, match=next(iter(bad))):
        train_utils.get_optimizer(cfg, params)


def test_get_optimizer_knows_lars_and_keeps_the_other_names():
    from ssv_amd.utils import train_utils
    params = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(_lib().SsvError, match="parameters on the GPU"):           # good settings: LARS gets as far as the arena, which has no CPU form
        train_utils.get_optimizer({"name": "lars", "lr": 0.6, "weight_decay": 1e-6}, params)
    with pytest.raises(NotImplementedError, match="Invalid optimizer lamb"):
        train_utils.get_optimizer({"name": "lamb", "lr": 0.6, "weight_decay": 1e-6}, params)
    with pytest.raises(NotImplementedError, match="adam"):
        train_utils.get_optimizer({"name": "adam", "lr": 0.6, "weight_decay": 1e-6}, params)


def test_lars_config_is_the_synthetic_simclr_config_with_the_lars_block():
    import yaml
    cfgs = os.path.join(ROOT, "self-supervised-vision_amd", "configs")
    base = yaml.safe_load(open(os.path.join(cfgs, "simclr_r50_224_synthetic.yaml")))
    lars = yaml.safe_load(open(os.path.join(cfgs, "simclr_r50_224_lars_synthetic.yaml")))
    assert lars["optimizer"] == {"name": "lars", "lr": 0.6, "weight_decay": 1.0e-06, "momentum": 0.9, "eta": 0.001}
    assert {k: v for k, v in lars.items() if k != "optimizer"} == {k: v for k, v in base.items() if k != "optimizer"}


def test_abi_version_and_graph_admission():
    lib = _lib()
    assert lib.ABI_VERSION == 124 and lib.load().ssv_version() == 124
    import inspect
    from ssv_amd import graph
    src = inspect.getsource(graph.StepGraph._why_not)
    assert "FusedLARS" in src and "neither the fused SGD" in src
