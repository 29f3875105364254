#!/usr/bin/env python3
"""What gaussian_blur adds to the GPU augmentation of a step, HIP-event timed after warm-up.
Measured: GpuTransform.draw + GpuTransform.apply for two views at B 512, source 256x256 -> 224x224 (the shape of
configs/simclr_r50_224_blur_synthetic.yaml), three chains that differ in the blur entry only:
  none   no gaussian_blur: the entry points and launches of a chain without blur - the yardstick;
  p0.5   gaussian_blur {sigma: [0.1, 2.0], apply_prob: 0.5}  (the config's);
  p1.0   gaussian_blur {sigma: [0.1, 2.0], apply_prob: 1.0}  (every view blurred).
The legs are timed in two alternated passes; the spread between the passes is the noise of the box.  Reported per blur leg: the added
milliseconds per step over `none`, the same as a fraction of a SimCLR ResNet-50 step (--step-ms: ms_per_step of a plain `python bench.py`
run on the same machine), and the time of a pure copy of the blur's HBM traffic (one uint8 write and one uint8 read of Ho*Wo*3 bytes per
blurred image; the fp32 output is written by the unblurred chain as well) at the device's measured copy rate.
    python tools/bench_blur.py [--step-ms MS] [--commit SHA] [--out profiles/blur_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SRC, OUT, STEPS = 512, (256, 256), (224, 224), 8
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _chain(blur):
    c = {"color_jitter": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4, "hue": 0.1, "apply_prob": 0.8}, "random_gray": {"p": 0.2},
         "random_resized_crop": {"size": list(OUT), "scale": [0.2, 1.0]}, "random_flip": None}
    if blur is not None:
        c["gaussian_blur"] = {"sigma": [0.1, 2.0], "apply_prob": blur}
    c.update({"to_tensor": None, "normalize": {"mean": MEAN, "std": STD}})
    return c


def _timed(fn, warmup, reps):
    import torch
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + i)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": reps}


def _commit():
    try:
        sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, timeout=20).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, timeout=20).stdout.strip()
        return (sha + ("+uncommitted" if dirty else "")) if sha else None
    except (OSError, subprocess.SubprocessError):
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--step-ms", type=float, default=None, help="ms_per_step of `python bench.py` (SimCLR ResNet-50, batch 512) on this machine")
    ap.add_argument("--commit", default=None, help="the tree's commit, where the tool runs from a copy without its history")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_bench.json"))
    args = ap.parse_args()
    import torch
    from ssv_amd import _lib
    from ssv_amd.utils import augmentations
    if not torch.cuda.is_available():
        raise SystemExit("bench_blur.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    n = B * STEPS
    images = torch.randint(0, 256, (n, SRC[0], SRC[1], 3), dtype=torch.uint8, generator=g).to(dev)
    order = torch.randperm(n, generator=g).to(dev)
    tfs = {"none": augmentations.get_transform(_chain(None)), "p0.5": augmentations.get_transform(_chain(0.5)), "p1.0": augmentations.get_transform(_chain(1.0))}
    blurred = {}

    def leg(name):
        tf = tfs[name]

        def fn(step):
            idx = order[(step % STEPS) * B:(step % STEPS + 1) * B]
            params = tf.draw(images, idx, step, 2)
            if name not in blurred and tf.blur is not None:
                blurred[name] = float((params[..., 15] > 0).float().mean().item())
            return tf.apply(images, idx, params)
        return fn

    first = {k: _timed(leg(k), 5, args.reps) for k in tfs}
    second = {k: _timed(leg(k), 2, args.reps) for k in reversed(list(tfs))}
    # the device's copy rate on a buffer of the staging image's size (read + write counted), for the traffic bound
    plane = OUT[0] * OUT[1] * 3
    a, b = torch.empty(2 * B * plane, dtype=torch.uint8, device=dev), torch.empty(2 * B * plane, dtype=torch.uint8, device=dev)
    copy = _timed(lambda i: b.copy_(a), 5, args.reps)
    copy_gbs = 2 * a.numel() / (copy["ms_median"] * 1e-3) / 1e9
    out = {"device": torch.cuda.get_device_name(0), "library_source_sha16": _lib.source_sha16(), "library_sha16": _lib.lib_sha16(), "commit": args.commit or _commit(),
           "workload": f"draw + apply, 2 views, B {B}, uint8 {SRC[0]}x{SRC[1]} -> fp32 {OUT[0]}x{OUT[1]}, HIP events, median of {args.reps} after warm-up, two alternated passes",
           "legs": {k: {"first_pass": first[k], "second_pass": second[k]} for k in tfs}, "blurred_fraction_of_first_batch": blurred,
           "device_copy_GBps_read_plus_write": round(copy_gbs, 1), "simclr_r50_step_ms": args.step_ms, "added": {}}
    base = min(first["none"]["ms_median"], second["none"]["ms_median"])
    noise = abs(first["none"]["ms_median"] - second["none"]["ms_median"])
    out["yardstick_ms"], out["yardstick_pass_to_pass_ms"] = base, round(noise, 4)
    for k, frac in (("p0.5", 0.5), ("p1.0", 1.0)):
        ms = min(first[k]["ms_median"], second[k]["ms_median"])
        bound_ms = 2 * (2 * B * frac) * plane / (copy_gbs * 1e9) * 1e3              # write + read of the staged uint8 image of every blurred view
        out["added"][k] = {"added_ms_per_step": round(ms - base, 4), "times_the_unblurred_chain": round(ms / base, 3),
                           "fraction_of_simclr_r50_step": None if not args.step_ms else round((ms - base) / args.step_ms, 5),
                           "traffic_bound_ms": round(bound_ms, 4), "added_over_traffic_bound": round((ms - base) / bound_ms, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
