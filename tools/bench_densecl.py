#!/usr/bin/env python3
"""DenseCL timings on the GPU, HIP-event timed after warm-up, the compared sides ALTERNATING call by call in one process; two passes (the spread between them is
the noise of the box); the measuring leg is a child process under its own time limit.
  queue_nce   ops.queue_nce (csrc/densecl.hip: loss and dq of InfoNCE against a queue with one gathered positive per query) at (m, K, d) = (8192, 4096, 128) - 16
              cells per image at batch 512 - and (25088, 65536, 128) - ResNet-50 at 224 x 224, batch 512 - on unit-norm Gaussian rows, temperature 0.2.  Sides: "fused"
              (bf16x3), "unfused" (the same entry point under arithmetic f32: scores and their gradient through the workspace), "torch" (matmul, logsumexp,
              softmax, matmul, in chunks of 4096 queries so that the logits fit) and "moco_route" (the existing MocoLoss composition on the gathered positives:
              ssv_conv2d_fwd -> ssv_moco_loss_fwd_bwd -> ssv_conv2d_dgrad with the m x K logits in memory).  Also how the sides agree.
  dense_match ops.dense_match at (b, cells, c) = (512, 16, 512) and (512, 49, 2048) on ReLU-of-Gaussian maps against torch normalize + bmm + argmax; GB/s against
              the bytes of the two maps.
  whole_step  DenseCL ResNet-18 (CIFAR stem), 32 x 32, batch 512 through the trainer, built from configs/densecl_r18_32_synthetic.yaml, beside the MoCo step with
              the same settings, their steps ALTERNATING, eager and as a step graph; the share of the DenseCL step spent in the two new calls (their median times at
              the step's shapes, measured between steps, over the step's).  --r50: ResNet-50, 224 x 224, batch 512 with 65,536-row queues, eager, or why it did not run.
    python tools/bench_densecl.py [--out profiles/densecl_bench.json] [--skip-step] [--r50]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 900
WARMUP, REPS = 20, 100
STEP_WARMUP, STEP_REPS = 4, 12
NCE_SHAPES = ((8192, 4096, 128), (25088, 65536, 128))
MATCH_SHAPES = ((512, 16, 512), (512, 49, 2048))
TEMPERATURE = 0.2
CONFIG = os.path.join(ROOT, "self-supervised-vision_amd", "configs", "densecl_r18_32_synthetic.yaml")


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


def queue_nce_leg(dev, m, K, d):
    import torch
    from ssv_amd import _lib, ops
    assert ops.ARITHMETIC == "bf16x3", "run without SSV_ARITHMETIC: the fused side is timed under the default arithmetic"
    q, keys, bank = _unit_rows(m, d, dev, 1), _unit_rows(m, d, dev, 2), _unit_rows(K, d, dev, 3)
    pos = torch.randperm(m, device=dev, generator=torch.Generator(device=dev).manual_seed(4)).to(torch.int32)
    it = 1.0 / TEMPERATURE
    kpos = keys.index_select(0, pos.long()).contiguous()                  # the gathered positives: handed to the two baselines ready-made

    def fused():
        return ops.queue_nce(q, keys, pos, bank, K, it)

    def unfused():
        with ops.arithmetic("f32"):
            return ops.queue_nce(q, keys, pos, bank, K, it)

    def composed(chunk=4096):
        loss, lses, dqs = 0.0, [], []
        for r0 in range(0, m, chunk):
            qc, kc = q[r0:r0 + chunk], kpos[r0:r0 + chunk]
            sp = (qc * kc).sum(dim=1, keepdim=True) * it
            sc = torch.cat([sp, (qc @ bank.T) * it], dim=1)
            lse = torch.logsumexp(sc, dim=1)
            p = torch.exp(sc - lse[:, None])
            dqs.append(((p[:, 1:] @ bank) + (p[:, :1] - 1.0) * kc) * (it / m))
            loss = loss + (lse - sp[:, 0]).sum()
            lses.append(lse)
        return loss / m, torch.cat(lses), torch.cat(dqs), None

    def moco_route():
        neg = ops.conv2d_fwd(q.view(m, 1, 1, d), bank).view(m, bank.shape[0])
        loss, dq = ops.moco_loss(q, kpos, neg, K, it)
        ops.conv2d_dgrad(neg.view(m, 1, 1, -1), bank, (m, 1, 1, d), addend=dq.view(m, 1, 1, d), out=dq.view(m, 1, 1, d))
        return loss, None, dq, None

    fns = {"fused": fused, "unfused": unfused, "torch": composed, "moco_route": moco_route}
    outs, refused = {}, {}
    for name in list(fns):
        try:
            outs[name] = fns[name]()
            torch.cuda.synchronize()
        except (_lib.SsvError, RuntimeError) as exc:                       # a baseline that does not take the shape is reported, not timed
            refused[name] = str(exc)[:300]
            del fns[name]
    rel = lambda a, b, i: round(float((outs[a][i] - outs[b][i]).norm() / outs[b][i].norm()), 9) if a in outs and b in outs else None
    res = {"m": m, "K": K, "d": d, "route": ops.queue_nce_route(d), "products_gflop": round(4.0 * m * K * d / 1e9, 3), "bank_mb": round(K * d * 4 / 1e6, 2),
           "logits_mb": round(m * K * 4 / 1e6, 2), "workspace_mb": {a: round(_lib.load().ssv_queue_nce_workspace_bytes(m, K, d, c) / 1e6, 2)
                                                                     for a, c in (("fused", _lib.ARITH_BF16X3), ("unfused", _lib.ARITH_F32_MFMA))},
           "flags": [int(outs[n][3].item()) for n in ("fused", "unfused")], "refused": refused,
           "relative_difference": {"dq_fused_vs_torch": rel("fused", "torch", 2), "dq_unfused_vs_torch": rel("unfused", "torch", 2), "lse_fused_vs_torch": rel("fused", "torch", 1),
                                   "dq_fused_vs_unfused": rel("fused", "unfused", 2), "dq_moco_route_vs_torch": rel("moco_route", "torch", 2)}}
    del outs
    torch.cuda.empty_cache()
    res["first_pass"], res["second_pass"] = _alternating(fns, WARMUP, REPS), _alternating(fns, 5, REPS)
    for p in ("first_pass", "second_pass"):
        r = res[p]
        for other in ("unfused", "torch", "moco_route"):
            if other in r:
                r[f"fused_over_{other}_median"] = round(r["fused"]["ms_median"] / r[other]["ms_median"], 4)
        r["fused_products_tflops"] = round(res["products_gflop"] / r["fused"]["ms_median"], 2)
    res["fused_not_slower_than_unfused"] = all(res[p]["fused_over_unfused_median"] <= 1.0 for p in ("first_pass", "second_pass"))
    return res


def dense_match_leg(dev, b, s, c):
    import torch
    from ssv_amd import ops
    g = torch.Generator(device=dev).manual_seed(11)
    f1, f2 = torch.relu(torch.randn(b, s, c, device=dev, generator=g)), torch.relu(torch.randn(b, s, c, device=dev, generator=g))
    base = (s * torch.arange(b, device=dev))[:, None]

    def ours():
        return ops.dense_match(f1, f2)

    def composed():
        n1, n2 = torch.nn.functional.normalize(f1, dim=2), torch.nn.functional.normalize(f2, dim=2)
        cos = torch.bmm(n1, n2.transpose(1, 2))
        sim, j = cos.max(dim=2)
        return (j + base).to(torch.int32), sim

    a, t = ours(), composed()
    torch.cuda.synchronize()
    res = {"b": b, "cells": s, "c": c, "maps_mb": round(2 * b * s * c * 4 / 1e6, 2), "products_gflop": round(2.0 * b * s * s * c / 1e9, 3),
           "cells_where_idx_differs_from_torch": int((a[0] != t[0]).sum()), "max_abs_sim_difference": float((a[1] - t[1]).abs().max())}
    fns = {"dense_match": ours, "torch": composed}
    res["first_pass"], res["second_pass"] = _alternating(fns, WARMUP, REPS), _alternating(fns, 5, REPS)
    for p in ("first_pass", "second_pass"):
        r = res[p]
        r["dense_match_over_torch_median"] = round(r["dense_match"]["ms_median"] / r["torch"]["ms_median"], 4)
        r["dense_match_gb_per_s"] = round(res["maps_mb"] / r["dense_match"]["ms_median"], 1)
    return res


def _build_pair(dev, cfg, arch, reduce_bottom_conv, n):
    import bench
    keys = ("proj_dim", "momentum", "queue_size", "loss_fn", "optimizer")
    bench.ALGOS.update(moco=("ssv_amd.models.moco", "MoCo"), densecl=("ssv_amd.models.densecl", "DenseCL"))
    bench.BENCH_CFG.update(moco={k: cfg[k] for k in keys}, densecl={k: cfg[k] for k in keys + ("densecl",)})
    try:
        return {name: bench.build(dev, name, steps_per_epoch=n, arch=arch, reduce_bottom_conv=reduce_bottom_conv)[0] for name in ("moco", "densecl")}
    finally:
        for name in ("moco", "densecl"):
            del bench.ALGOS[name], bench.BENCH_CFG[name]


def _views(dev, batch, size):
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    base = 2.0 * torch.nn.functional.interpolate(torch.randn(batch, 3, 4, 4, device=dev, generator=g), size=size, mode="bilinear", align_corners=False)
    return {"aug_1": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g), "aug_2": base + 0.3 * torch.randn(batch, 3, size, size, device=dev, generator=g),
            "label": torch.zeros(batch)}


def _new_calls(dev, t, batch, res_key_eager, res_key_graph):
    """the two new calls at the step's own shapes, between steps"""
    import torch
    from ssv_amd import ops
    fmap = t.query_encoder.last_map
    cells, c, d = fmap.shape[1] * fmap.shape[2], fmap.shape[3], t.config["proj_dim"]
    g = torch.Generator(device=dev).manual_seed(13)
    f1, f2 = torch.relu(torch.randn(fmap.shape, device=dev, generator=g)), torch.relu(torch.randn(fmap.shape, device=dev, generator=g))
    q, k = _unit_rows(batch * cells, d, dev, 9), _unit_rows(batch * cells, d, dev, 10)
    pos = ops.dense_match(f1, f2)[0].view(-1)
    it = 1.0 / t.config["loss_fn"]["temperature"]
    r = _alternating({"dense_match": lambda: ops.dense_match(f1, f2), "queue_nce": lambda: ops.queue_nce(q, k, pos, t.dense_bank.bank, t.dense_bank.size, it)}, WARMUP, REPS)
    both = r["dense_match"]["ms_median"] + r["queue_nce"]["ms_median"]
    out = {"cells": cells, "channels": c, "queries": batch * cells, "dense_queue": t.dense_bank.size, "route": ops.queue_nce_route(d), "dense_match": r["dense_match"],
           "queue_nce": r["queue_nce"], "share_of_eager_step": round(both / res_key_eager, 5)}
    if res_key_graph:
        out["share_of_graph_step"] = round(both / res_key_graph, 5)
    return out


def whole_step_leg(dev, batch=512, size=32):
    import yaml
    from ssv_amd import ops
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["data"]["batch_size"] == batch and cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    steps = _build_pair(dev, cfg, "resnet18", True, cfg["data"]["synthetic"]["num_train"])
    data, last = _views(dev, batch, size), {}

    def runner(name, graph):
        tr = steps[name].trainer

        def fn():
            last[f"{name}_{'graph' if graph else 'eager'}"] = (tr.step(data) if graph else tr.train_step(data))["loss"]
        return fn

    res = {"workload": f"resnet18 (CIFAR stem) {size}x{size}, batch {batch}; moco: proj {cfg['proj_dim']}, queue {cfg['queue_size']}, {cfg['loss_fn']}, SGD; densecl: the same plus "
                       f"the dense term, {cfg['densecl']}",
           "timing": "host clock around each step with a device synchronisation"}
    for mode, graph in (("eager", False), ("graph", True)):
        fns = {name: runner(name, graph) for name in steps}
        first, second = _alternating(fns, STEP_WARMUP, STEP_REPS, wall=True), _alternating(fns, 2, STEP_REPS, wall=True)
        res[mode] = {"first_pass": first, "second_pass": second,
                     "densecl_over_moco_median": [round(p["densecl"]["ms_median"] / p["moco"]["ms_median"], 4) for p in (first, second)]}
    res["step_graph"] = {name: steps[name].trainer._step_graph.describe() for name in steps}
    res["last_loss"] = last
    assert all(v == v for v in last.values()), f"a loss is NaN: {last}"
    t = steps["densecl"].trainer
    ops.check_queue_nce_flag(t.dense_loss_fn.last_flag)
    res["new_calls_in_step"] = _new_calls(dev, t, batch, res["eager"]["first_pass"]["densecl"]["ms_median"], res["graph"]["first_pass"]["densecl"]["ms_median"])
    return res


def r50_leg(dev, batch=512, size=224, queue=65536):
    """ResNet-50 at 224 x 224, batch 512, both queues 65,536 rows, eager: 25,088 dense queries per step.  Whatever stops it is reported in its place."""
    import torch
    import yaml
    cfg = yaml.safe_load(open(CONFIG))
    cfg["queue_size"], cfg["densecl"] = queue, {"loss_lambda": 0.5, "dense_queue_size": queue}
    try:
        steps = _build_pair(dev, cfg, "resnet50", False, 1000)
        data, last = _views(dev, batch, size), {}

        def runner(name):
            tr = steps[name].trainer

            def fn():
                last[name] = tr.train_step(data)["loss"]
            return fn
        timed = _alternating({name: runner(name) for name in steps}, 3, 8, wall=True)
        res = {"workload": f"resnet50 {size}x{size}, batch {batch}, queues of {queue} rows, eager", "steps": timed, "last_loss": last,
               "densecl_over_moco_median": round(timed["densecl"]["ms_median"] / timed["moco"]["ms_median"], 4),
               "peak_memory_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
        res["new_calls_in_step"] = _new_calls(dev, steps["densecl"].trainer, batch, timed["densecl"]["ms_median"], None)
        return res
    except Exception as exc:                                               # out of memory, a refused shape: the report says which
        return {"workload": f"resnet50 {size}x{size}, batch {batch}, queues of {queue} rows", "did_not_run": f"{type(exc).__name__}: {str(exc)[:400]}"}


def leg(skip_step, r50):
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"default_arithmetic": ops.ARITHMETIC, "queue_nce": [queue_nce_leg(dev, *s) for s in NCE_SHAPES], "dense_match": [dense_match_leg(dev, *s) for s in MATCH_SHAPES]}
    torch.cuda.empty_cache()
    if not skip_step:
        out["whole_step"] = whole_step_leg(dev)
    if r50:
        torch.cuda.empty_cache()
        out["whole_step_resnet50"] = r50_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--skip-step", action="store_true", help="the kernel measurements only")
    ap.add_argument("--r50", action="store_true", help="also the ResNet-50 / 224 x 224 / batch 512 step with 65,536-row queues")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densecl_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg(args.skip_step, args.r50)))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_densecl.py measures on the GPU; none is visible")
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16()}
    cmd = [sys.executable, os.path.abspath(__file__), "--leg"] + (["--skip-step"] if args.skip_step else []) + (["--r50"] if args.r50 else [])
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
