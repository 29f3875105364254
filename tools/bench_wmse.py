#!/usr/bin/env python3
"""W-MSE timings on the GPU, the compared sides ALTERNATING call by call in one process; two passes (the spread between them is the noise of the box); the
measuring leg is a child process under its own time limit.
  whitening   ops.whiten_fwd + ops.whiten_bwd (csrc/whiten.hip: one workgroup per sub-batch, one launch per direction) at (blocks, w, d) = (8, 128, 64) - batch
              512 x 2 views - and (4, 256, 128), for w_iter 1 and 4 (one call pair per iteration, fresh random blocks each), HIP-event timed after warm-up, medians
              of 200 calls, beside a plain torch composition on the same GPU: gather, centring, covariance, batched torch.linalg.cholesky, solve_triangular and bmm
              under autograd.  If torch's batched Cholesky is unavailable the error is recorded instead.  The fused kernel is reported as it is, slower legs included.
  whole_step  ResNet-18 (CIFAR stem), 32 x 32, batch 512 through the trainers: W-MSE (configs/wmse_r18_32_synthetic.yaml's hyper-parameters) beside SimCLR (bench.py's),
              their steps ALTERNATING, eager (train_step) and replayed as a step graph (step), wall-clock per step with a device synchronisation (at this size the
              host's enqueue time is part of the eager step); and the share of the W-MSE step spent in the whitening (its median time at the step's shape over the
              step's).
    python tools/bench_wmse.py [--out profiles/wmse_bench.json] [--skip-step]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 540
WARMUP, REPS = 20, 200
STEP_WARMUP, STEP_REPS = 12, 40
SHAPES = ((8, 128, 64), (4, 256, 128))
ITERS = (1, 4)
CONFIG = os.path.join(ROOT, "self-supervised-vision_amd", "configs", "wmse_r18_32_synthetic.yaml")


def _stats(times):
    times = sorted(times)
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": len(times)}


def _alternating(fns, warmup, reps, wall=False):
    """every function once per round; HIP events around each call, or (wall) the host clock around the call and a device synchronisation"""
    import torch
    times = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            if wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            if i >= warmup:
                times[k].append(ms)
    return {k: _stats(t) for k, t in times.items()}


def whitening_leg(dev, blocks, w, d, iters):
    import torch
    from ssv_amd import ops
    g = torch.Generator(device=dev).manual_seed(blocks + w + d)
    n = blocks * w
    mix = torch.eye(d, device=dev) + 0.3 * torch.randn(d, d, device=dev, generator=g) / d ** 0.5
    x = (torch.randn(n, d, device=dev, generator=g) @ mix + 1.0).contiguous()
    dy = torch.randn(n, d, device=dev, generator=g)
    rows = [torch.randperm(n, device=dev, generator=g).to(torch.int32).view(blocks, w).contiguous() for _ in range(iters)]
    eye = torch.eye(d, device=dev).expand(blocks, d, d)

    def fused():
        out = None
        for r in rows:
            y, mean, winv, _ = ops.whiten_fwd(x, r, 0.0)
            dx = ops.whiten_bwd(x, r, 0.0, mean, winv, dy)
            out = dx if out is None else out + dx
        return out

    def torch_composition():
        xin = x.detach().requires_grad_(True)
        total = 0.0
        for r in rows:
            xb = xin[r.long()]                                            # [blocks, w, d]
            xc = xb - xb.mean(dim=1, keepdim=True)
            s = xc.transpose(1, 2) @ xc / (w - 1)
            winv = torch.linalg.solve_triangular(torch.linalg.cholesky(s), eye, upper=False)
            total = total + ((xc @ winv.transpose(1, 2)).reshape(n, d) * dy).sum()
        return torch.autograd.grad(total, xin)[0]

    res = {"blocks": blocks, "w": w, "d": d, "w_iter": iters, "linalg_library": str(torch.backends.cuda.preferred_linalg_library())}
    a = fused()
    fns = {"fused": fused}
    try:
        b = torch_composition()
        torch.cuda.synchronize()
        res["max_abs_difference_of_dx"] = float((a - b).abs().max())
        res["max_abs_dx"] = float(b.abs().max())
        fns["torch"] = torch_composition
    except Exception as e:                                                # noqa: BLE001 - recorded, not hidden: the baseline is what this box's torch offers
        res["torch_composition_failed"] = f"{type(e).__name__}: {e}"[:400]
    res["first_pass"], res["second_pass"] = _alternating(fns, WARMUP, REPS), _alternating(fns, 5, REPS)
    if "torch" in fns:
        for p in ("first_pass", "second_pass"):
            res[p]["fused_over_torch_median"] = round(res[p]["fused"]["ms_median"] / res[p]["torch"]["ms_median"], 3)
    # the two directions apart (one iteration)
    y, mean, winv, _ = ops.whiten_fwd(x, rows[0], 0.0)
    res["directions"] = _alternating({"fwd": lambda: ops.whiten_fwd(x, rows[0], 0.0), "bwd": lambda: ops.whiten_bwd(x, rows[0], 0.0, mean, winv, dy)}, WARMUP, REPS)
    return res


def whole_step_leg(dev, batch=512, size=32):
    import torch
    import yaml
    import bench
    from ssv_amd import ops
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["data"]["batch_size"] == batch and cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    bench.ALGOS["wmse"] = ("ssv_amd.models.wmse", "WMSE")
    bench.BENCH_CFG["wmse"] = {k: cfg[k] for k in ("emb_dim", "head_hidden_dim", "loss_fn", "optimizer")}
    try:
        steps = {name: bench.build(dev, name, arch="resnet18", reduce_bottom_conv=True)[0] for name in ("simclr", "wmse")}
    finally:
        del bench.ALGOS["wmse"], bench.BENCH_CFG["wmse"]
    g = torch.Generator(device=dev).manual_seed(7)
    base = 2.0 * torch.nn.functional.interpolate(torch.randn(batch, 3, 4, 4, device=dev, generator=g), size=size, mode="bilinear", align_corners=False)
    data = {"aug_1": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g),
            "aug_2": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g), "label": torch.zeros(batch)}
    last = {}

    def runner(name, graph):
        t = steps[name].trainer

        def fn():
            last[f"{name}_{'graph' if graph else 'eager'}"] = (t.step(data) if graph else t.train_step(data))["loss"]
        return fn

    res = {"workload": f"resnet18 (CIFAR stem) {size}x{size}, batch {batch}; wmse: head {cfg['head_hidden_dim']}-{cfg['emb_dim']}, {cfg['loss_fn']}, AdamW; simclr: bench.py's (SGD)",
           "timing": "host clock around each step with a device synchronisation"}
    for mode, graph in (("eager", False), ("graph", True)):
        fns = {name: runner(name, graph) for name in steps}
        first, second = _alternating(fns, STEP_WARMUP, STEP_REPS, wall=True), _alternating(fns, 2, STEP_REPS, wall=True)
        res[mode] = {"first_pass": first, "second_pass": second,
                     "wmse_over_simclr_median": [round(p["wmse"]["ms_median"] / p["simclr"]["ms_median"], 4) for p in (first, second)]}
    res["step_graph"] = {name: steps[name].trainer._step_graph.describe() for name in steps}
    res["last_loss"] = last
    assert all(v == v for v in last.values()), f"a loss is NaN: {last}"
    d, w = cfg["emb_dim"], cfg["loss_fn"]["w_size"]
    blocks = 2 * (batch // w)
    x = torch.randn(2 * batch, d, device=dev, generator=g)
    dy = torch.randn(blocks * w, d, device=dev, generator=g)
    rows = torch.randperm(2 * batch, device=dev, generator=g).to(torch.int32).view(blocks, w).contiguous()

    def pair():
        y, mean, winv, _ = ops.whiten_fwd(x, rows, 0.0)
        ops.whiten_bwd(x, rows, 0.0, mean, winv, dy)

    wh = _alternating({"whiten": pair}, WARMUP, REPS)["whiten"]
    res["whitening_in_step"] = dict(wh, share_of_eager_step=round(wh["ms_median"] / res["eager"]["first_pass"]["wmse"]["ms_median"], 5),
                                    share_of_graph_step=round(wh["ms_median"] / res["graph"]["first_pass"]["wmse"]["ms_median"], 5))
    return res


def leg(skip_step):
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"default_arithmetic": ops.ARITHMETIC, "whitening": [whitening_leg(dev, *s, it) for s in SHAPES for it in ITERS]}
    torch.cuda.empty_cache()
    if not skip_step:
        out["whole_step"] = whole_step_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--skip-step", action="store_true", help="the whitening measurements only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wmse_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg(args.skip_step)))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_wmse.py measures on the GPU; none is visible")
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
