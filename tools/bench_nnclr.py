#!/usr/bin/env python3
"""NNCLR timings on the GPU, HIP-event timed after warm-up, the compared sides ALTERNATING call by call in one process; two passes (the spread between them is the
noise of the box); the measuring leg is a child process under its own time limit.
  lookup      ops.nn_lookup (csrc/nnlookup.hip: top-1 search fused into the product + gather, out_scale 1 / 0.1) at (m, n, d) = (1024, 98304, 256) and
              (1024, 16384, 128) on unit-norm Gaussian rows, beside what the library offered before it: ops.knn_search(k = 1) + index_select + scale.  Three sides:
              "fused" (bf16x3), "unfused" (the same entry point under arithmetic f32: the product through the workspace) and "baseline" (bf16x3, the default).
              Also: how the sides agree on idx, and the bank bytes per second of the fused call against the chip's measured float4 copy rate.
  whole_step  NNCLR ResNet-50, 224 x 224, batch 512 through the trainer, built from configs/nnclr_r50_224_synthetic.yaml (queue 98,304 x 256), beside the SimCLR step
              of bench.py, their steps ALTERNATING; median step time and images/s of each, and the share of the NNCLR step spent in the lookup (the lookup's median
              time at the step's shape, measured between steps, over the step's).
    python tools/bench_nnclr.py [--out profiles/nnclr_bench.json] [--skip-step]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 540
WARMUP, REPS = 20, 200
STEP_WARMUP, STEP_REPS = 3, 8
SHAPES = ((1024, 98304, 256), (1024, 16384, 128))
TEMPERATURE = 0.1
COPY_RATE_TBS = 6.29          # measured float4 copy rate of the MI355X (tools/bench_kmeans.py)
CONFIG = os.path.join(ROOT, "self-supervised-vision_amd", "configs", "nnclr_r50_224_synthetic.yaml")


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


def _unit_rows(rows, d, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(rows, d, device=dev, generator=g), dim=1)


def lookup_leg(dev, m, n, d):
    import torch
    from ssv_amd import ops
    bank, queries = _unit_rows(n, d, dev, 1), _unit_rows(m, d, dev, 2)
    scale = 1.0 / TEMPERATURE
    scale_dev = torch.full((), scale, device=dev)

    assert ops.ARITHMETIC == "bf16x3", "run without SSV_ARITHMETIC: the fused side and the baseline are timed under the default arithmetic"

    def fused():
        return ops.nn_lookup(queries, bank, out_scale=scale)

    def unfused():
        with ops.arithmetic("f32"):
            return ops.nn_lookup(queries, bank, out_scale=scale)

    def baseline():
        sim, idx = ops.knn_search(queries, bank, 1)
        return bank.index_select(0, idx[:, 0].long()) * scale_dev, idx[:, 0], sim[:, 0]

    outs = {k: fn() for k, fn in (("fused", fused), ("unfused", unfused), ("baseline", baseline))}
    torch.cuda.synchronize()
    same = lambda a, b: round(float((outs[a][1].long() == outs[b][1].long()).float().mean().item()), 6)
    res = {"m": m, "n": n, "d": d, "product_gflop": round(2.0 * m * n * d / 1e9, 2), "bank_mb": round(n * d * 4 / 1e6, 1),
           "idx_agreement": {"fused_vs_baseline": same("fused", "baseline"), "fused_vs_unfused": same("fused", "unfused")},
           "nn_rows_equal_where_idx_agrees": bool(torch.equal(outs["fused"][0][outs["fused"][1] == outs["baseline"][1]], outs["baseline"][0][outs["fused"][1] == outs["baseline"][1]]))}
    fns = {"fused": fused, "baseline": baseline, "unfused": unfused}
    res["first_pass"], res["second_pass"] = _alternating(fns, WARMUP, REPS), _alternating(fns, 5, REPS)
    for p in ("first_pass", "second_pass"):
        r = res[p]
        r["fused_over_baseline_median"] = round(r["fused"]["ms_median"] / r["baseline"]["ms_median"], 3)
        r["fused_over_unfused_median"] = round(r["fused"]["ms_median"] / r["unfused"]["ms_median"], 3)
        r["fused_product_tflops"] = round(res["product_gflop"] / r["fused"]["ms_median"], 1)
        tbs = n * d * 4 / (r["fused"]["ms_median"] * 1e-3) / 1e12
        r["fused_bank_tb_per_s"] = round(tbs, 3)                 # the bank's bytes ONCE over the call's time (the kernel streams it once per block of 256 queries)
        r["fused_bank_share_of_copy_rate"] = round(tbs / COPY_RATE_TBS, 3)
    res["fused_not_slower_than_baseline"] = all(res[p]["fused_over_baseline_median"] <= 1.0 for p in ("first_pass", "second_pass"))
    return res


def whole_step_leg(dev, batch=512, size=224):
    import torch
    import yaml
    import bench
    from ssv_amd import ops
    cfg = yaml.safe_load(open(CONFIG))
    assert cfg["data"]["batch_size"] == batch and cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    bench.ALGOS["nnclr"] = ("ssv_amd.models.nnclr", "NNCLR")
    bench.BENCH_CFG["nnclr"] = {k: cfg[k] for k in ("proj_dim", "proj_hidden_dim", "pred_hidden_dim", "queue_size", "queue_seed", "loss_fn", "optimizer")}
    try:
        steps = {name: bench.build(dev, name)[0] for name in ("simclr", "nnclr")}
    finally:
        del bench.ALGOS["nnclr"], bench.BENCH_CFG["nnclr"]
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
    res = {"workload": f"resnet50 {size}x{size}, batch {batch}, trainer.train_step; nnclr: projector {cfg['proj_hidden_dim']}-{cfg['proj_dim']}, predictor {cfg['pred_hidden_dim']}, "
                       f"queue {cfg['queue_size']}, T {cfg['loss_fn']['temperature']}, SGD; simclr: bench.py's",
           "first_pass": first, "second_pass": second, "last_loss": last}
    for p in (first, second):
        for name in steps:
            p[name]["images_per_s"] = round(batch / (p[name]["ms_median"] * 1e-3), 1)
    res["nnclr_over_simclr_median"] = [round(p["nnclr"]["ms_median"] / p["simclr"]["ms_median"], 4) for p in (first, second)]
    res["spread_between_passes"] = {n: round(abs(first[n]["ms_median"] - second[n]["ms_median"]) / first[n]["ms_median"], 4) for n in steps}
    # the lookup of the step, on the trainer's own queue and at its shape (2 x batch queries), timed between steps
    t = steps["nnclr"].trainer
    queries = _unit_rows(2 * batch, cfg["proj_dim"], dev, 3)
    look = _alternating({"lookup": lambda: ops.nn_lookup(queries, t.memory_bank.get_vectors(), n=t.memory_bank.size, out_scale=1.0 / t.loss_fn.temperature)}, WARMUP, REPS)["lookup"]
    res["lookup_in_step"] = dict(look, share_of_step=round(look["ms_median"] / first["nnclr"]["ms_median"], 5))
    return res


def leg(skip_step):
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    out = {"default_arithmetic": ops.ARITHMETIC, "temperature": TEMPERATURE, "copy_rate_tb_per_s": COPY_RATE_TBS, "lookup": [lookup_leg(dev, *s) for s in SHAPES]}
    torch.cuda.empty_cache()
    if not skip_step:
        out["whole_step"] = whole_step_leg(dev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--skip-step", action="store_true", help="the lookup measurements only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnclr_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg(args.skip_step)))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_nnclr.py measures on the GPU; none is visible")
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
