#!/usr/bin/env python3
"""PCL timings on the GPU, HIP-event timed after warm-up, the compared sides ALTERNATING call by call in one process; two passes (the spread between them is the
noise of the box); the measuring leg is a child process under its own time limit.
  kernel      ops.proto_nce (csrc/protonce.hip: loss and dq of the ProtoNCE term in one pass) at (m, K per segment, segments, d) = (256, 1000, 3, 128),
              (512, 4096, 3, 128) and (512, 65536, 1, 128) - the last beyond what the trainer can ask for (k-means stops at 4096 clusters): the traffic regime - on
              unit-norm Gaussian rows with 1 / phi log-uniform in [2, 20].  Three sides: "fused" (bf16x3), "unfused" (the same entry point under arithmetic f32:
              scores and their gradient through the workspace) and "torch" (per segment matmul, scale, logsumexp, softmax, matmul).  Also how the sides agree.
  whole_step  PCL ResNet-18 (CIFAR stem), 32 x 32, batch 512 through the trainer, built from configs/pcl_r18_32_synthetic.yaml with random unit prototypes in
              place of an E-step (no loader here), beside the MoCo step with the same settings, their steps ALTERNATING, eager and as a step graph; and the share of
              the PCL step spent in the ProtoNCE call (its median time at the step's shape, measured between steps, over the step's).
    python tools/bench_pcl.py [--out profiles/pcl_bench.json] [--skip-step]"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 540
WARMUP, REPS = 20, 100
STEP_WARMUP, STEP_REPS = 4, 12
SHAPES = ((256, 1000, 3, 128), (512, 4096, 3, 128), (512, 65536, 1, 128))
CONFIG = os.path.join(ROOT, "self-supervised-vision_amd", "configs", "pcl_r18_32_synthetic.yaml")


def _stats(times):
    times = sorted(times)
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": len(times)}


def _alternating(fns, warmup, reps, wall=False):
    """every function once per round; HIP events around each call, or (``wall``: whole steps, which synchronise themselves) the host clock"""
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


def _unit_rows(rows, d, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(rows, d, device=dev, generator=g), dim=1)


def _problem(dev, m, k, segs, d):
    import torch
    g = torch.Generator(device=dev).manual_seed(3)
    q, protos = _unit_rows(m, d, dev, 1), _unit_rows(k * segs, d, dev, 2)
    inv_phi = torch.exp(torch.rand(k * segs, device=dev, generator=g) * math.log(10.0) + math.log(2.0))
    labels = torch.randint(0, k, (segs, m), device=dev, generator=g).to(torch.int32)
    return q, protos, inv_phi, labels, tuple(k * (s + 1) for s in range(segs))


def kernel_leg(dev, m, k, segs, d):
    import torch
    from ssv_amd import ops
    q, protos, inv_phi, labels, seg_end = _problem(dev, m, k, segs, d)
    assert ops.ARITHMETIC == "bf16x3", "run without SSV_ARITHMETIC: the fused side is timed under the default arithmetic"
    rows = torch.arange(m, device=dev)
    lab64 = labels.long()

    def fused():
        return ops.proto_nce(q, protos, inv_phi, labels, seg_end)

    def unfused():
        with ops.arithmetic("f32"):
            return ops.proto_nce(q, protos, inv_phi, labels, seg_end)

    def composed():
        loss, dq, lses, b = 0.0, 0.0, [], 0
        for s, e in enumerate(seg_end):
            c, ip = protos[b:e], inv_phi[b:e]
            sc = (q @ c.T) * ip
            lse = torch.logsumexp(sc, dim=1)
            p = torch.exp(sc - lse[:, None])
            p[rows, lab64[s]] -= 1.0
            dq = dq + (p * ip) @ c
            loss = loss + (lse - sc[rows, lab64[s]]).mean()
            lses.append(lse)
            b = e
        return loss / segs, torch.stack(lses), dq / (segs * m), None

    outs = {name: fn() for name, fn in (("fused", fused), ("unfused", unfused), ("torch", composed))}
    torch.cuda.synchronize()
    rel = lambda a, b, i: round(float((outs[a][i] - outs[b][i]).norm() / outs[b][i].norm()), 9)
    res = {"m": m, "k_per_segment": k, "segments": segs, "d": d, "route": ops.proto_nce_route(d), "products_gflop": round(4.0 * m * k * segs * d / 1e9, 3),
           "prototypes_mb": round(k * segs * d * 4 / 1e6, 2), "scores_mb": round(m * k * segs * 4 / 1e6, 2), "flags": [int(outs[n][3].item()) for n in ("fused", "unfused")],
           "relative_difference": {"dq_fused_vs_torch": rel("fused", "torch", 2), "dq_unfused_vs_torch": rel("unfused", "torch", 2), "lse_fused_vs_torch": rel("fused", "torch", 1),
                                   "dq_fused_vs_unfused": rel("fused", "unfused", 2)}}
    fns = {"fused": fused, "unfused": unfused, "torch": composed}
    res["first_pass"], res["second_pass"] = _alternating(fns, WARMUP, REPS), _alternating(fns, 5, REPS)
    for p in ("first_pass", "second_pass"):
        r = res[p]
        r["fused_over_unfused_median"] = round(r["fused"]["ms_median"] / r["unfused"]["ms_median"], 3)
        r["fused_over_torch_median"] = round(r["fused"]["ms_median"] / r["torch"]["ms_median"], 3)
        r["fused_products_tflops"] = round(res["products_gflop"] / r["fused"]["ms_median"], 2)
    res["fused_not_slower_than_unfused"] = all(res[p]["fused_over_unfused_median"] <= 1.0 for p in ("first_pass", "second_pass"))
    return res


def whole_step_leg(dev, batch=512, size=32):
    import torch
    import yaml
    import bench
    from ssv_amd import ops
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["data"]["batch_size"] == batch and cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    n = cfg["data"]["synthetic"]["num_train"]
    keys = ("proj_dim", "momentum", "queue_size", "loss_fn", "optimizer")
    bench.ALGOS.update(moco=("ssv_amd.models.moco", "MoCo"), pcl=("ssv_amd.models.pcl", "PCL"))
    bench.BENCH_CFG.update(moco={k: cfg[k] for k in keys}, pcl={k: cfg[k] for k in keys + ("pcl",)})
    try:
        steps = {name: bench.build(dev, name, steps_per_epoch=n, arch="resnet18", reduce_bottom_conv=True)[0] for name in ("moco", "pcl")}
    finally:
        for name in ("moco", "pcl"):
            del bench.ALGOS[name], bench.BENCH_CFG[name]
    t = steps["pcl"].trainer
    g = torch.Generator(device=dev).manual_seed(7)
    # in place of an E-step (there is no loader): random unit prototypes, every concentration at its mean, random cluster labels
    t.prototypes.copy_(_unit_rows(t.seg_end[-1], cfg["proj_dim"], dev, 5))
    t.inv_phi.fill_(1.0 / cfg["pcl"]["temperature"])
    for s, k in enumerate(t.num_clusters):
        t.cluster_labels[s].copy_(torch.randint(0, k, (n,), device=dev, generator=g).to(torch.int32))
    t.proto_on = True
    base = 2.0 * torch.nn.functional.interpolate(torch.randn(batch, 3, 4, 4, device=dev, generator=g), size=size, mode="bilinear", align_corners=False)
    data = {"aug_1": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g), "aug_2": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g),
            "index": torch.randperm(n, device=dev, generator=g)[:batch].contiguous(), "label": torch.zeros(batch)}
    last = {}

    def runner(name, graph):
        tr = steps[name].trainer

        def fn():
            last[f"{name}_{'graph' if graph else 'eager'}"] = (tr.step(data) if graph else tr.train_step(data))["loss"]
        return fn

    res = {"workload": f"resnet18 (CIFAR stem) {size}x{size}, batch {batch}; moco: proj {cfg['proj_dim']}, queue {cfg['queue_size']}, {cfg['loss_fn']}, SGD; pcl: the same plus "
                       f"ProtoNCE over {cfg['pcl']['num_clusters']} random unit prototypes",
           "timing": "host clock around each step with a device synchronisation"}
    for mode, graph in (("eager", False), ("graph", True)):
        fns = {name: runner(name, graph) for name in steps}
        first, second = _alternating(fns, STEP_WARMUP, STEP_REPS, wall=True), _alternating(fns, 2, STEP_REPS, wall=True)
        res[mode] = {"first_pass": first, "second_pass": second,
                     "pcl_over_moco_median": [round(p["pcl"]["ms_median"] / p["moco"]["ms_median"], 4) for p in (first, second)]}
    res["step_graph"] = {name: steps[name].trainer._step_graph.describe() for name in steps}
    res["last_loss"] = last
    assert all(v == v for v in last.values()), f"a loss is NaN: {last}"
    ops.check_proto_nce_flag(t.proto_loss_fn.last_flag)
    q = _unit_rows(batch, cfg["proj_dim"], dev, 9)
    labels = t.cluster_labels.index_select(1, data["index"])
    pn = _alternating({"proto_nce": lambda: ops.proto_nce(q, t.prototypes, t.inv_phi, labels, t.seg_end)}, WARMUP, REPS)["proto_nce"]
    res["proto_nce_in_step"] = dict(pn, route=ops.proto_nce_route(cfg["proj_dim"]),
                                    share_of_eager_step=round(pn["ms_median"] / res["eager"]["first_pass"]["pcl"]["ms_median"], 5),
                                    share_of_graph_step=round(pn["ms_median"] / res["graph"]["first_pass"]["pcl"]["ms_median"], 5))
    return res


def leg(skip_step):
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"default_arithmetic": ops.ARITHMETIC, "kernel": [kernel_leg(dev, *s) for s in SHAPES]}
    torch.cuda.empty_cache()
    if not skip_step:
        out["whole_step"] = whole_step_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--skip-step", action="store_true", help="the kernel measurements only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcl_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg(args.skip_step)))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcl.py measures on the GPU; none is visible")
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
