#!/usr/bin/env python3
"""VICReg timings on the GPU, HIP-event timed after warm-up, two passes (the spread between them is the noise of the box); the measuring leg is a child process
under its own time limit.
  loss        utils.losses.VicregLoss forward + backward (prep, two weight-gradient GEMMs, cgrad, two forward GEMMs with the addend, two scales) at
              (B 512, D 2048) and (B 512, D 8192) in both arithmetics, beside a plain torch composition of the paper's lines with autograd on the same GPU in the
              same process (fp32 matmul), their calls ALTERNATING; then the fused call's time and scopes per profiling class from the library's own events.  The two
              results are compared on the same inputs before anything is timed.  GEMM FLOP of the loss from the shapes: 4 products of 2 B D^2 each.
  whole_step  VICReg ResNet-50, 224 x 224, batch 512 through the trainer, built from configs/vicreg_r50_224_lars_synthetic.yaml (expander 8192, LARS), beside the
              Barlow Twins step of bench.py (expander 4096, SGD), their steps ALTERNATING in the same call; median step time and images/s of each, both passes.
    python tools/bench_vicreg.py [--out profiles/vicreg_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 540
WARMUP, REPS = 10, 50
PROF_CALLS = 20
STEP_WARMUP, STEP_REPS = 3, 8
SHAPES = ((512, 2048), (512, 8192))
CONFIG = os.path.join(ROOT, "self-supervised-vision_amd", "configs", "vicreg_r50_224_lars_synthetic.yaml")


def _stats(times):
    times = sorted(times)
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": len(times)}


def _alternating(fns, warmup, reps):
    """every function once per round, HIP events around each call"""
    import torch
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: _stats(t) for k, t in times.items()}


def torch_lines(x, y, sim_coeff=25.0, std_coeff=25.0, cov_coeff=1.0, eps=1e-4):
    """the paper's pseudocode in plain torch"""
    import torch
    b, d = x.shape
    sim = torch.nn.functional.mse_loss(x, y)
    xc, yc = x - x.mean(dim=0), y - y.mean(dim=0)
    sx, sy = torch.sqrt(xc.var(dim=0) + eps), torch.sqrt(yc.var(dim=0) + eps)
    std = torch.relu(1 - sx).mean() / 2 + torch.relu(1 - sy).mean() / 2
    cx, cy = (xc.T @ xc) / (b - 1), (yc.T @ yc) / (b - 1)
    off = lambda c: c.pow(2).sum() - torch.diagonal(c).pow(2).sum()
    cov = off(cx) / d + off(cy) / d
    return sim_coeff * sim + std_coeff * std + cov_coeff * cov


def loss_leg(dev, b, d):
    import torch
    from ssv_amd import _lib, ops
    from ssv_amd.utils import losses
    g = torch.Generator(device=dev).manual_seed(11)
    scale = torch.tensor([0.25, 4.0], device=dev).repeat(d // 2)                 # the hinge active on half the columns
    x = (torch.randn(b, d, device=dev, generator=g) * scale).requires_grad_(True)
    y = (x.detach() + 0.1 * torch.randn(b, d, device=dev, generator=g) * scale).requires_grad_(True)
    fn = losses.VicregLoss()

    def fused():
        x.grad = y.grad = None
        fn(x, y).backward()

    def composed():
        x.grad = y.grad = None
        torch_lines(x, y).backward()

    res = {"B": b, "D": d, "gemm_gflop": round(4 * 2 * b * d * d / 1e9, 2)}
    composed()
    ref = (torch_lines(x, y).item(), x.grad.clone(), y.grad.clone())
    for arith in ("bf16x3", "f32"):
        with ops.arithmetic(arith):
            fused()
            got = fn(x, y).item()
            rel = lambda a_, r: float((a_ - r).norm() / r.norm())
            res[f"agreement_{arith}"] = {"loss_fused": got, "loss_torch": ref[0], "dx_rel_l2": rel(x.grad, ref[1]), "dy_rel_l2": rel(y.grad, ref[2])}
            fns = {"fused": fused, "torch": composed}
            res[arith] = {"first_pass": _alternating(fns, WARMUP, REPS), "second_pass": _alternating(fns, 3, REPS)}
            for p in ("first_pass", "second_pass"):
                r = res[arith][p]
                r["fused_over_torch_median"] = round(r["fused"]["ms_median"] / r["torch"]["ms_median"], 3)
                r["fused_gemm_tflops"] = round(res["gemm_gflop"] / r["fused"]["ms_median"], 1)
    # where the fused call's time goes, from the library's own per-class HIP events (a run of its own: the events serialise the launches)
    with ops.arithmetic("bf16x3"):
        fused()
        torch.cuda.synchronize()
        _lib.prof_enable(True)
        _lib.prof_reset()
        for _ in range(PROF_CALLS):
            fused()
        torch.cuda.synchronize()
        cls = _lib.prof_collect()
        _lib.prof_enable(False)
    res["fused_classes_bf16x3"] = {k: {"ms_per_call": round(ms / PROF_CALLS, 4), "launches_per_call": n / PROF_CALLS} for k, (ms, n) in cls.items() if n}
    return res


def whole_step_leg(dev, batch=512, size=224):
    import torch
    import yaml
    import bench
    from ssv_amd.utils import train_utils
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["data"]["batch_size"] == batch and cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    bench.ALGOS["vicreg"] = ("ssv_amd.models.vicreg", "VICReg")
    bench.BENCH_CFG["vicreg"] = {"proj_dim": cfg["proj_dim"], "loss_fn": cfg["loss_fn"], "optimizer": cfg["optimizer"]}
    try:
        steps = {name: bench.build(dev, name)[0] for name in ("barlow", "vicreg")}
    finally:
        del bench.ALGOS["vicreg"], bench.BENCH_CFG["vicreg"]
    assert isinstance(steps["vicreg"].trainer.optim, train_utils.FusedLARS)
    # two noisy views of one smooth random image per sample: samples that differ at low spatial frequencies, as real images do
    g = torch.Generator(device=dev).manual_seed(7)
    base = 2.0 * torch.nn.functional.interpolate(torch.randn(batch, 3, 7, 7, device=dev, generator=g), size=size, mode="bilinear", align_corners=False)
    data = {"aug_1": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g),
            "aug_2": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g), "label": torch.zeros(batch)}
    last = {}

    def runner(name):
        def fn():
            last[name] = steps[name](data)
            assert last[name] == last[name], f"{name}: the loss is NaN"
        return fn

    fns = {name: runner(name) for name in steps}
    first, second = _alternating(fns, STEP_WARMUP, STEP_REPS), _alternating(fns, 1, STEP_REPS)
    res = {"workload": f"resnet50 {size}x{size}, batch {batch}, trainer.train_step; vicreg: expander {cfg['proj_dim']}, LARS; barlow: expander 4096, SGD",
           "first_pass": first, "second_pass": second, "last_loss": last}
    for p in (first, second):
        for name in steps:
            p[name]["images_per_s"] = round(batch / (p[name]["ms_median"] * 1e-3), 1)
    res["vicreg_over_barlow_median"] = [round(p["vicreg"]["ms_median"] / p["barlow"]["ms_median"], 4) for p in (first, second)]
    res["spread_between_passes"] = {n: round(abs(first[n]["ms_median"] - second[n]["ms_median"]) / first[n]["ms_median"], 4) for n in steps}
    return res


def leg(skip_step):
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"default_arithmetic": ops.ARITHMETIC, "loss": [loss_leg(dev, b, d) for b, d in SHAPES]}
    torch.cuda.empty_cache()
    if not skip_step:
        out["whole_step"] = whole_step_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--skip-step", action="store_true", help="the loss measurements only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vicreg_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg(args.skip_step)))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_vicreg.py measures on the GPU; none is visible")
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16()}
    cmd = [sys.executable, os.path.abspath(__file__), "--leg"] + (["--skip-step"] if args.skip_step else [])
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_SECONDS + 30)
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
