#!/usr/bin/env python3
"""LARS timings on the GPU, HIP-event timed after warm-up, 200 calls per figure, two passes (the spread between them is the noise of the box); the measuring leg
is a child process under its own time limit.
  update      the optimizer update alone on the REAL arenas of ResNet-18 (reduce_bottom_conv) and ResNet-50, each with the SimCLR projector, two gradient slabs:
              ssv_lars_step (two launches) beside ssv_sgd_nesterov on the same arena (one launch: the update the other recipes run, the baseline) and beside a
              LARS composed of torch._foreach calls over flat per-tensor views of the same buffers (no guard for zero norms: it does less).  Bytes per parameter
              from the shapes: LARS 36 with two slabs (12 read by the norms pass, 24 moved by the update), SGD 24; over the medians, beside the measured float4
              copy rate of the chip, 6.29 TB/s.  The learning rate is 1e-6 so that 400 updates of the same gradients leave the arena where it was.
  whole_step  SimCLR ResNet-50, 224 x 224, batch 512 through the trainer (bench.build), one trainer with `sgd` and one with `lars`, their steps ALTERNATING in the
              same call; median step time of each, both passes.
    python tools/bench_lars.py [--out profiles/lars_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 420
COPY_RATE_TBS = 6.29          # measured float4 copy rate of the MI355X (8.0 TB/s on paper)
WARMUP, REPS = 20, 200
STEP_WARMUP, STEP_REPS = 3, 10
LARS_CFG = {"name": "lars", "lr": 0.6, "weight_decay": 1e-6, "momentum": 0.9, "eta": 0.001}
BYTES = {"lars": 36, "sgd_nesterov": 24}


def _timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": reps}


def update_leg(dev, arch):
    import torch
    from ssv_amd import _lib
    from ssv_amd.models import heads
    from ssv_amd.networks import resnet
    from ssv_amd.utils import train_utils
    torch.manual_seed(420)
    if arch == "resnet18":
        enc, dim = resnet.resnet18(reduce_bottom_conv=True).to(dev), 512
    else:
        enc, dim = resnet.resnet50(reduce_bottom_conv=False).to(dev), 2048
    head = heads.SimclrProjectionHead(dim, 128).to(dev)
    params = list(enc.parameters()) + list(head.parameters())
    opt = train_utils.get_optimizer(dict(LARS_CFG, lr=1e-6), params)
    a = opt.arena
    a.grad.copy_(1e-2 * torch.randn(a.numel, device=dev))
    a.grad_alt.copy_(1e-2 * torch.randn(a.numel, device=dev))
    nparam = sum(p.numel() for p in params)
    lr, wd, mom, eta = opt.hyper()

    def lars():
        opt.step()

    def sgd_nesterov():
        _lib.call("ssv_sgd_nesterov", a.numel, _lib.ptr(a.data), _lib.ptr(a.grad), _lib.ptr(a.grad_alt), _lib.ptr(opt.momentum_buffer), lr, wd, mom, 0, _lib.stream())

    seg = lambda flat: [flat[o:o + p.numel()] for o, p in zip(a.offsets, params)]
    ps, gs, g2s, mus = seg(a.data), seg(a.grad), seg(a.grad_alt), seg(opt.momentum_buffer)
    on = [i for i, p in enumerate(params) if p.dim() > 1]

    def foreach_lars():
        u = torch._foreach_add(gs, g2s)
        ua, pa = [u[i] for i in on], [ps[i] for i in on]
        torch._foreach_add_(ua, pa, alpha=wd)
        q = torch._foreach_div(torch._foreach_mul(torch._foreach_norm(pa), eta), torch._foreach_norm(ua))
        torch._foreach_mul_(ua, q)
        torch._foreach_mul_(mus, mom)
        torch._foreach_add_(mus, u)
        torch._foreach_add_(ps, mus, alpha=-lr)

    res = {"arch": arch, "tensors": len(params), "adapted_tensors": len(on), "params": nparam, "arena_floats": a.numel, "chunks": opt._chunks,
           "bytes_per_param": dict(BYTES)}
    legs = (("lars", lars), ("sgd_nesterov", sgd_nesterov), ("foreach_lars", foreach_lars))
    for name, fn in legs:
        res[name] = _timed(fn, WARMUP, REPS)
    for name, fn in legs:
        res[name + "_second_pass"] = _timed(fn, 5, REPS)          # alternated second pass
    for name in BYTES:
        tbs = BYTES[name] * nparam / (res[name]["ms_median"] * 1e-3) / 1e12
        res[name + "_tb_per_s"] = round(tbs, 3)
        res[name + "_share_of_copy_rate"] = round(tbs / COPY_RATE_TBS, 3)
    res["lars_over_sgd_nesterov_median"] = round(res["lars"]["ms_median"] / res["sgd_nesterov"]["ms_median"], 3)
    res["foreach_over_lars_median"] = round(res["foreach_lars"]["ms_median"] / res["lars"]["ms_median"], 2)
    assert torch.isfinite(a.data).all() and torch.isfinite(opt.trust_ratios()).all()
    del opt, params, enc, head
    torch.cuda.empty_cache()
    return res


def whole_step_leg(dev, batch=512, size=224):
    import torch
    import bench
    from ssv_amd.utils import train_utils
    steps = {}
    for name in ("sgd", "lars"):
        saved = bench.BENCH_CFG["simclr"]["optimizer"]
        if name == "lars":
            bench.BENCH_CFG["simclr"]["optimizer"] = dict(LARS_CFG)
        try:
            steps[name], _ = bench.build(dev, "simclr")
        finally:
            bench.BENCH_CFG["simclr"]["optimizer"] = saved
    assert isinstance(steps["lars"].trainer.optim, train_utils.FusedLARS) and isinstance(steps["sgd"].trainer.optim, train_utils.FusedSGD)
    # two noisy views of one smooth random image per sample: samples that differ at low spatial frequencies, as real images do
    g = torch.Generator(device=dev).manual_seed(7)
    base = 2.0 * torch.nn.functional.interpolate(torch.randn(batch, 3, 7, 7, device=dev, generator=g), size=size, mode="bilinear", align_corners=False)
    data = {"aug_1": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g),
            "aug_2": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g), "label": torch.zeros(batch)}

    def run(reps, warmup):
        times = {"sgd": [], "lars": []}
        for i in range(warmup + reps):
            for name in ("sgd", "lars"):                      # alternating: both see the same clocks and the same neighbours
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                loss = steps[name](data)
                b.record()
                b.synchronize()
                if i >= warmup:
                    times[name].append(a.elapsed_time(b))
                assert loss == loss, f"{name}: the loss is NaN"
        out = {}
        for name, t in times.items():
            t.sort()
            out[name] = {"ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3), "reps": len(t)}
        return out

    first, second = run(STEP_REPS, STEP_WARMUP), run(STEP_REPS, 1)
    res = {"workload": f"SimCLR resnet50 {size}x{size}, batch {batch}, trainer.train_step", "first_pass": first, "second_pass": second}
    res["lars_over_sgd_median"] = [round(p["lars"]["ms_median"] / p["sgd"]["ms_median"], 4) for p in (first, second)]
    res["spread_between_passes"] = {n: round(abs(first[n]["ms_median"] - second[n]["ms_median"]) / first[n]["ms_median"], 4) for n in ("sgd", "lars")}
    return res


def leg():
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"arithmetic": ops.ARITHMETIC, "copy_rate_tb_per_s": COPY_RATE_TBS, "update": [update_leg(dev, arch) for arch in ("resnet18", "resnet50")]}
    out["whole_step"] = whole_step_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lars_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg()))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_lars.py measures on the GPU; none is visible")
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16()}
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg"], capture_output=True, text=True, timeout=LEG_SECONDS + 30)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"the measuring leg failed (rc {res.returncode})")
    out.update(json.loads(lines[-1][len("RESULT "):]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
