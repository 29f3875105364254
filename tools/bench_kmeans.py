#!/usr/bin/env python3
"""k-means timings on the GPU, HIP-event timed after warm-up, 200 calls per figure, two passes (the spread between them is the noise of the box); the measuring leg
is a child process under its own time limit.
  assign     ops.kmeans_assign alone (the centroid-side operands are made inside the call, as a caller with fresh centroids pays it), beside a baseline composed
             ONLY of entry points that predate it: ops.conv2d_fwd for X C^T - 1/2 |c|^2 into HBM (the half norms ride as the GEMM's bias, made outside the
             timed region), torch.argmax over its rows, torch.bincount.  The baseline produces neither the distances nor the objective.
  iteration  one full Lloyd iteration: kmeans_assign on the operands the last update left + kmeans_update; baseline: the three calls above, then
             torch one_hot, ops.conv2d_wgrad for onehot^T X, a division by the counts.
Shapes (n, d, k): (50000, 512, 10), (50000, 2048, 100), (200000, 128, 1024).  x_bytes_per_s: the bytes of x (counted once; the kernel reads them once per 256 centroids and once more for the distances) over the median, beside the
measured float4 copy rate of the chip, 6.29 TB/s.
    python tools/bench_kmeans.py [--out profiles/kmeans_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 420
SHAPES = ((50000, 512, 10), (50000, 2048, 100), (200000, 128, 1024))
COPY_RATE_TBS = 6.29          # measured float4 copy rate of the MI355X (8.0 TB/s on paper)
WARMUP, REPS = 20, 200


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


def leg():
    import torch
    from ssv_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for n, d, k in SHAPES:
        g = torch.Generator().manual_seed(n + d + k)
        centres = torch.randn(k, d, generator=g)
        x = (centres[torch.randint(0, k, (n,), generator=g)] + 2.0 * torch.randn(n, d, generator=g)).to(dev)
        c0 = x[torch.randperm(n, generator=g)[:k].to(dev)].contiguous()
        cent, prep = c0.clone(), ops.kmeans_prep(x, c0)
        cent_b = c0.clone()
        x4 = x.view(n, 1, 1, d)

        def assign():
            return ops.kmeans_assign(x, c0)

        def assign_baseline(c=c0, bias=(-0.5 * (c0 * c0).sum(1)).contiguous()):
            scores = ops.conv2d_fwd(x4, c, bias=bias).view(n, k)
            labels = torch.argmax(scores, dim=1)
            return labels, torch.bincount(labels, minlength=k)

        state = {"ready": False}

        def iteration():
            labels, _, counts, _ = ops.kmeans_assign(x, cent, prep=prep, prep_ready=state["ready"])
            ops.kmeans_update(x, labels, counts, cent, prep=prep)
            state["ready"] = True

        kp = (k + 3) // 4 * 4
        sums = torch.empty(kp, d, device=dev)

        def iteration_baseline():
            bias = -0.5 * (cent_b * cent_b).sum(1)
            labels, counts = assign_baseline(cent_b, bias)
            onehot = torch.nn.functional.one_hot(labels, kp).to(torch.float32)
            ops.conv2d_wgrad(x4, onehot.view(n, 1, 1, kp), sums, sums, accumulate=False)
            keep = (counts == 0).unsqueeze(1)
            cent_b.copy_(torch.where(keep, cent_b, sums[:k] / counts.clamp(min=1).unsqueeze(1)))
            ops.invalidate_weight_caches()

        la, lb = assign()[0], assign_baseline()[0]
        agree = float((la.long() == lb).float().mean().item())
        if agree < 0.999:
            raise SystemExit(f"fused and composed assignments agree on only {agree:.4%} of the rows at {(n, d, k)}")
        res = {"n": n, "d": d, "k": k, "label_agreement_with_baseline": round(agree, 6)}
        for name, fn in (("assign", assign), ("assign_baseline", assign_baseline), ("iteration", iteration), ("iteration_baseline", iteration_baseline)):
            res[name] = _timed(fn, WARMUP, REPS)
        for name, fn in (("assign", assign), ("assign_baseline", assign_baseline), ("iteration", iteration), ("iteration_baseline", iteration_baseline)):
            res[name + "_second_pass"] = _timed(fn, 5, REPS)          # alternated second pass
        res["assign_speedup_median"] = round(res["assign_baseline"]["ms_median"] / res["assign"]["ms_median"], 2)
        res["iteration_speedup_median"] = round(res["iteration_baseline"]["ms_median"] / res["iteration"]["ms_median"], 2)
        passes = (k + 255) // 256
        tbs = 4.0 * n * d / (res["assign"]["ms_median"] * 1e-3) / 1e12
        res["assign_x_tb_per_s"] = round(tbs, 3)
        res["assign_x_share_of_copy_rate"] = round(tbs / COPY_RATE_TBS, 3)
        res["assign_x_passes"] = passes
        res["assign_product_tflops"] = round(2.0 * n * d * k / (res["assign"]["ms_median"] * 1e-3) / 1e12, 2)
        rows.append(res)
    return {"arithmetic": ops.ARITHMETIC, "copy_rate_tb_per_s": COPY_RATE_TBS, "shapes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg()))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py measures on the GPU; none is visible")
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
