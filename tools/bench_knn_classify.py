#!/usr/bin/env python3
"""Weighted kNN classifier timings on the GPU (ops.knn_search + ops.knn_vote, csrc/knnclassify.hip), HIP-event timed after a 20-call warm-up, medians of up to
200 calls, two alternated passes (the spread between them is the noise of the box); the measuring leg is a child process under its own time limit.
A figure whose call takes more than 10 ms is the median of FEWER calls - as many as fit 2 s, at least 10; every figure carries its own "reps".
  whole      knn_search + knn_vote (the vote reads its device flag: one synchronisation inside the timed region), beside a baseline composed ONLY of what
             predates them: ops.conv2d_fwd for S = Q B^T into HBM (row chunks under the GEMM's 2^29-element limit), torch.topk, a gather of the labels,
             exp((sim - sim[:, :1]) / T), scatter_add_ into [m, C], argmax.  The baseline is not tuned.
  search     knn_search alone, with the library's partition and with chunk_rows in {256, 1024, 4096}.
  classes    per call of knn_search, from the library's own per-class HIP events (ssv_prof_*): "product" = the conv_fwd class (the GEMM), "selection" = the misc
             class (knn_select_k, knn_merge_k and, under bf16x3, the split of the bank's planes).
  vote       knn_vote alone.
Shapes (m, n, d, k, C): m 10,000 x n 50,000 at d 128 / 512 / 2048 with k 20 and 200, C 10; m 10,000 x n 200,000, d 128, k 200, C 1000.
    python tools/bench_knn_classify.py [--out profiles/knn_classify_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEG_SECONDS = 900
SHAPES = tuple((10000, 50000, d, k, 10) for d in (128, 512, 2048) for k in (20, 200)) + ((10000, 200000, 128, 200, 1000),)
CHUNK_ROWS = (256, 1024, 4096)
TEMPERATURE = 0.07
WARMUP, REPS, SLOW_MS, SLOW_BUDGET_MS, MIN_REPS = 20, 200, 10.0, 2000.0, 10


def _timed(fn, warmup=WARMUP):
    import torch

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    fn()
    pilot = once()
    slow = pilot > SLOW_MS
    reps = max(MIN_REPS, min(REPS, int(SLOW_BUDGET_MS / pilot))) if slow else REPS
    for _ in range(2 if slow else warmup):
        fn()
    torch.cuda.synchronize()
    times = sorted(once() for _ in range(reps))
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": reps}


def leg():
    import torch
    from ssv_amd import _lib, ops
    dev = torch.device("cuda:0")
    rows = []
    made = {}
    for m, n, d, k, c in SHAPES:
        if (n, d, c) not in made:
            made.clear()
            g = torch.Generator().manual_seed(n + d + c)
            centres = torch.randn(c, d, generator=g)
            yb = torch.randint(0, c, (n,), generator=g)
            yq = torch.randint(0, c, (m,), generator=g)
            unit = lambda y: torch.nn.functional.normalize(centres[y] + 0.3 * d ** 0.5 * torch.randn(y.numel(), d, generator=g), dim=1).to(dev)
            made[(n, d, c)] = (unit(yb), yb.to(dev), unit(yq))
        bank, labels, queries = made[(n, d, c)]
        labels32 = labels.to(torch.int32)
        q4 = queries.view(m, 1, 1, d)
        rows_per = min(m, ((1 << 29) - (1 << 23)) // n)

        def search(cr=0):
            return ops.knn_search(queries, bank, k, chunk_rows=cr)

        sim0, idx0 = search()

        def vote():
            return ops.knn_vote(sim0, idx0, labels32, c, TEMPERATURE)

        def whole():
            return ops.knn_vote(*search(), labels32, c, TEMPERATURE)

        def baseline():
            preds = []
            for r0 in range(0, m, rows_per):
                s = ops.conv2d_fwd(q4[r0:r0 + rows_per], bank).view(-1, n)
                sim, idx = torch.topk(s, k, dim=1)
                w = torch.exp((sim - sim[:, :1]) / TEMPERATURE)
                scores = torch.zeros(sim.shape[0], c, device=dev).scatter_add_(1, labels[idx], w)
                preds.append(scores.argmax(1))
            return torch.cat(preds)

        agree = float((whole()[:, 0].long() == baseline()).float().mean().item())
        if agree < 0.99:
            raise SystemExit(f"the classifier and the composed baseline agree on only {agree:.4%} of the queries at {(m, n, d, k, c)}")
        res = {"m": m, "n": n, "d": d, "k": k, "C": c, "prediction_agreement_with_baseline": round(agree, 6), "baseline_row_chunks": -(-m // rows_per)}
        legs = [("whole", whole), ("baseline", baseline), ("search", search), ("vote", vote)] + [(f"search_chunk_rows_{cr}", lambda cr=cr: search(cr)) for cr in CHUNK_ROWS]
        for name, fn in legs:
            res[name] = _timed(fn)
        for name, fn in legs[:3]:
            res[name + "_second_pass"] = _timed(fn, warmup=5)          # alternated second pass
        _lib.prof_enable(True)
        _lib.prof_reset()
        for _ in range(5):
            search()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(False)
        res["classes_ms_per_search"] = {"product": round(prof["conv_fwd"][0] / 5, 4), "selection": round(prof["misc"][0] / 5, 4),
                                        "launches": {"product": prof["conv_fwd"][1] // 5, "selection": prof["misc"][1] // 5}}
        res["whole_speedup_median"] = round(res["baseline"]["ms_median"] / res["whole"]["ms_median"], 2)
        res["product_tflops"] = round(2.0 * m * n * d / (res["classes_ms_per_search"]["product"] * 1e-3) / 1e12, 1)
        res["selection_s_gb_per_s"] = round(4.0 * m * n / (res["classes_ms_per_search"]["selection"] * 1e-3) / 1e9, 1)   # bytes of S over the selection's time: one pass' worth
        rows.append(res)
        sys.stderr.write(json.dumps(res) + "\n")
    return {"arithmetic": ops.ARITHMETIC, "temperature": TEMPERATURE, "shapes": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_classify_bench.json"))
    args = ap.parse_args()
    if args.leg:
        print("RESULT " + json.dumps(leg()))
        return 0
    import torch
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_classify.py measures on the GPU; none is visible")
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16()}
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg"], stdout=subprocess.PIPE, text=True, timeout=LEG_SECONDS + 30)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        sys.stderr.write(res.stdout[-2000:])
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
