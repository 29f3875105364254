#!/usr/bin/env python3
"""PIRL timings on the GPU, HIP-event timed after warm-up; every leg is a child process under its own time limit, and a leg that fails ends the run.
  step  ms/step of configs/pirl.yaml's regime (resnet18 reduce_bottom_conv, 32x32, batch 256, 4 patches of 16x16, K 1000, N 50000), eager
  loss  ssv_pirl_loss_fwd_bwd alone at (B 256, K 1000, N 50000) and (B 1024, K 32003, N 200000), D 128, beside a baseline composed ONLY of entry points that
        predate it: torch index_select gathers of the positive / negative rows, ops.l2norm_fwd, ops.conv2d_fwd for the B x K product, the MoCo rows kernel
        once per cross-entropy.  The baseline stops at the loss value and the soft-max weights: it produces neither d img nor d patch (no entry point gives
        them), so it does LESS than the fused call it is compared with.
    python tools/bench_pirl.py [--out profiles/pirl_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = {"loss": 240, "step": 300}
D = 128


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


def leg_loss():
    import torch
    import torch.nn.functional as F
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for b, k, n in ((256, 1000, 50000), (1024, 32003, 200000)):
        g = torch.Generator().manual_seed(b)
        bank = F.normalize(torch.randn(n, D, generator=g), dim=1).to(dev)
        img, patch = torch.randn(b, D, generator=g).to(dev), torch.randn(b, D, generator=g).to(dev)
        perm = torch.randperm(n, generator=g)
        pos, neg = perm[:b].to(dev), perm[b:b + k].to(dev)
        inv_t, w = 1.0 / 0.07, 0.5
        k16 = (k + 15) // 16 * 16
        neg_rows = torch.zeros(k16, D, device=dev)

        def fused():
            return ops.pirl_loss(bank, pos, neg, img, patch, True, inv_t, w)

        def composed():
            pos_rows = bank.index_select(0, pos)
            torch.index_select(bank, 0, neg, out=neg_rows[:k])
            ops.invalidate_weight_caches()                              # the negatives change every step: a cached image of the GEMM operand is stale
            vi, _ = ops.l2norm_fwd(img, True)
            vp, _ = ops.l2norm_fwd(patch, True)
            logits = ops.conv2d_fwd(pos_rows.view(b, 1, 1, D), neg_rows).view(b, k16)
            logits_2 = logits.clone()                                   # the rows kernel overwrites its logits
            l1, _ = ops.moco_loss(pos_rows, vp, logits, k, inv_t)
            l2, _ = ops.moco_loss(pos_rows, vi, logits_2, k, inv_t)
            return w * l1 + (1.0 - w) * l2

        lf, lc = float(fused()[0].item()), float(composed().item())
        if abs(lf - lc) > 1e-4 * abs(lf):
            raise SystemExit(f"fused {lf} and composed {lc} losses disagree at B {b} K {k}")
        tf, tc = _timed(fused, 20, 200), _timed(composed, 20, 200)
        tf2, tc2 = _timed(fused, 5, 200), _timed(composed, 5, 200)      # a second, alternated pass: the spread between passes is the noise of this box
        rows.append({"B": b, "K": k, "N": n, "D": D, "splits": int(ops._lib.load().ssv_pirl_default_splits(b, k)), "loss_fused": lf, "loss_composed": lc,
                     "fused": tf, "composed_baseline": tc, "fused_second_pass": tf2, "composed_second_pass": tc2,
                     "speedup_median": round(tc["ms_median"] / tf["ms_median"], 2),
                     "fused_product_tflops": round(2.0 * b * k * D / (tf["ms_median"] * 1e-3) / 1e12, 2)})
    return {"loss_entry_point": rows}


def leg_step():
    import torch
    from ssv_amd.models.pirl import PIRL
    from ssv_amd.utils import train_utils
    dev = torch.device("cuda:0")
    n, bs, k = 50000, 256, 1000

    class Loader:
        shape = (n, 32, 32, 3)

        def __len__(self):
            return (n + bs - 1) // bs

        def eval_batches(self):
            g = torch.Generator(device=dev).manual_seed(1)
            for s in range(0, n, bs):
                e = min(n, s + bs)
                yield {"index": torch.arange(s, e, device=dev), "img": torch.randn(e - s, 3, 32, 32, device=dev, generator=g)}

    t = object.__new__(PIRL)
    t.config = {"epochs": 1000, "encoder": {"reduce_bottom_conv": True}, "scheduler": {"name": "cosine", "warmup_epochs": 0}, "proj_dim": D, "patch_size": 16,
                "num_patches": 4, "num_negatives": k, "momentum": 0.5, "optimizer": {"name": "sgd", "lr": 0.01, "weight_decay": 1e-4},
                "loss_fn": {"normalize": True, "temperature": 0.07, "loss_weight": 0.5}}
    t.device, t.train_loader, t.logger = dev, Loader(), types.SimpleNamespace(print=lambda *a, **kw: None)
    torch.manual_seed(420)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t._build("resnet18")
    b.record()
    b.synchronize()
    init_ms = a.elapsed_time(b)
    t.scheduler, t.warmup_epochs = train_utils.get_scheduler({**t.config["scheduler"], "epochs": 1000}, optimizer=t.optim)
    g = torch.Generator().manual_seed(2)
    batches = [{"index": torch.randperm(n, generator=g)[:bs].to(dev), "aug_1": torch.randn(bs, 3, 32, 32, generator=g).to(dev),
                "aug_2": torch.randn(bs, 3, 32, 32, generator=g).to(dev)} for _ in range(4)]
    state = {"i": 0, "loss": None}

    def step():
        state["loss"] = t.train_step(batches[state["i"] % len(batches)])["loss"]
        state["i"] += 1
    timing = _timed(step, 10, 60)
    return {"train_step": {"workload": f"PIRL resnet18 (reduce_bottom_conv) 32x32 bs {bs}, 4 patches of 16x16, K {k}, N {n}, the loss read every step", "eager": timing,
                           "images_per_s": round(bs / (timing["ms_median"] * 1e-3), 1), "bank_initialisation_ms": round(init_ms, 1), "last_loss": state["loss"]}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", choices=tuple(LEG_SECONDS), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pirl_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps({"loss": leg_loss, "step": leg_step}[args.leg]()))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_pirl.py measures on the GPU; none is visible")
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16()}
    for leg, seconds in LEG_SECONDS.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True, timeout=seconds + 30,
                             env=dict(os.environ, WANDB_MODE="disabled"))
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"leg {leg} failed (rc {res.returncode}): nothing further is started")
        out.update(json.loads(lines[-1][len("RESULT "):]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
