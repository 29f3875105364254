#!/usr/bin/env python3
"""bench.py - images/sec of the SimCLR (default; --algo byol|barlow for the siblings) ResNet-50 two-view training step on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1: starts its N ranks itself, one process per GPU, and relays rank 0's line)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W             (the same ranks started by an outer launcher)

One "step" = the reference train_step (models/simclr.py:86-95) on one per-GPU batch: two views ->
ResNet-50 (std 7x7/2 stem) + projector forward with per-view BatchNorm -> NT-Xent over the GLOBAL batch
(RCCL all-gather of the embeddings) -> backward -> gradient all-reduce -> SGD-Nesterov -> loss.item().
Inputs are synthetic and resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline line.  ``--full`` adds everything else the line can carry, each
after the timed region: the per-kernel-class roofline, the arithmetic block and the fp32-instruction leg, config 3's per-rank emulation, the
collective timing of a multi-rank run, the CPU baseline with its parity gates, config 1, the kNN leg and the BYOL / DINO legs.
``--dump-outputs DIR`` writes what the last timed step left its caller (loss, parameters) as .npy files: builds compare output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    # `python bench.py --gpus N` with N > 1 and no process group in the environment: this process becomes the waiting parent of N ranks
    # (python -m torch.distributed.run ... bench.py <same arguments>) and exits with their code.  Standard library only up to here -
    # the parent never imports torch, never touches HIP (ssv_amd/launch.py says why).
    from ssv_amd import launch as _launch
    _launch.maybe_spawn_ranks(os.path.abspath(__file__), sys.argv[1:], _launch.gpus_flag(sys.argv[1:]))

import torch  # noqa: E402

# rocprofv3 --pmc passes aggregated by tools/pmc_traffic.py / tools/pmc_mfma.py (tools/profile_step.sh) and the per-layer operand-stream table of
# tools/bench_conv.py.  Each file records the build it was measured on (src_sha16 = ssv_source_sha16() of the profiled library); counters of another
# build are NOT replayed: the line then carries traffic: null and counters_stale: true.
PMC_FILES = {"simclr": "r06_simclr_b%d_pmc_hbm_traffic.json", "dino": "r06_dino_b%d_pmc_hbm_traffic.json"}
CONV_LAYER_FILE = "r06_conv_layers_b%d.csv"
PMC_MFMA_FILES = {"simclr": "r06_simclr_b%d_pmc_mfma.json", "dino": "r06_dino_b%d_pmc_mfma.json"}
FP32_MFMA_PEAK_TFLOPS = 157.3        # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0       # MI355X_MICROARCH.md: dense bf16 MFMA (never the 2:1-sparsity headline)
BF16X3_TERMS = 6                     # bf16 piece products per fp32 product in the shipped arithmetic (csrc/split_bf16.h)
BF16X3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / BF16X3_TERMS            # 416.7 TFLOP/s of fp32 products: the roof of the pipe the dominant kernels run on
HBM_PEAK_GBS = 8000.0


def arithmetic_block(device):
    """What `dtype: f32` means in this line: fp32 operands and results; each fp32 product evaluated as six exact bf16 piece products accumulated in fp32 on the
    bf16 matrix pipe (csrc/split_bf16.h).  The error ratios are measured HERE, on this device: a forward-, data-gradient- and weight-gradient-shaped product of a
    ResNet-50 bottleneck (28 x 28 x 512 -> 128, batch 32) in both arithmetics against an fp64 evaluation - tests/test_gpu_split.py holds every one of the 53 layers
    x 3 products to <= 1.05."""
    from ssv_amd import _lib, ops
    n, h, c, k = 32, 28, 512, 128
    g = torch.Generator(device=device).manual_seed(7)
    x = torch.relu(torch.randn(n, h, h, c, device=device, generator=g) + 0.3)
    w = (torch.randn(k, c, 1, 1, device=device, generator=g) * (2.0 / c) ** 0.5).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, h, h, k, device=device, generator=g)
    xd, wd, dyd = x.reshape(-1, c).double(), w.reshape(k, c).double(), dy.reshape(-1, k).double()
    ref = (xd @ wd.t(), dyd @ wd, dyd.t() @ xd)
    err = {}
    for name in ("f32", "bf16x3"):
        with ops.arithmetic(name):
            y = ops.conv2d_fwd(x, w, 1, 0)
            dx = ops.conv2d_dgrad(dy, w, tuple(x.shape), 1, 0)
            dw = torch.zeros_like(w)
            ops.conv2d_wgrad(x, dy, w, dw, 1, 0, accumulate=False)
            torch.cuda.synchronize()
            got = (y.reshape(-1, k), dx.reshape(-1, c), dw.reshape(k, c))
            err[name] = [float((a.double() - r).norm() / r.norm()) for a, r in zip(got, ref)]
    ratios = [b / a for a, b in zip(err["f32"], err["bf16x3"])]
    return {"name": ops.ARITHMETIC, "operands": "fp32 (HBM, LDS staging input)", "results": "fp32",
            "product": "a*b = sum of %d of the 9 products of three bf16 pieces per operand (a = a0+a1+a2 exact, round to nearest even); every piece product is exact" % BF16X3_TERMS,
            "terms": BF16X3_TERMS, "accumulate": "fp32 (v_mfma_f32_16x16x32_bf16; a0b0 and the five small terms in separate accumulators, added in the epilogue)",
            "instruction": "v_mfma_f32_16x16x32_bf16" if ops.ARITHMETIC == "bf16x3" else "v_mfma_f32_32x32x2_f32",
            "error_vs_fp64": {"shape": "28x28x512 -> 128 1x1, batch 32: forward, data gradient, weight gradient (relative l2)",
                              "fp32_mfma": [float("%.3e" % e) for e in err["f32"]], "bf16x3": [float("%.3e" % e) for e in err["bf16x3"]],
                              "worst_ratio_bf16x3_over_fp32_mfma": round(max(ratios), 3), "bar": 1.05,
                              "all_53_layers_x_3_products": "tests/test_gpu_split.py::test_all_53_layer_shapes_x_3_products_no_worse_than_fp32_mfma"},
            "not_on_this_arithmetic": "the 3-channel image stem (forward, weight gradient), the strided data-gradient kernel (three 3x3 / stride-2 layers), attention and "
                                      "NT-Xent Gram products run on v_mfma_f32_32x32x2_f32 (ssv_conv_arithmetic() reports per launch)",
            "switch": "SSV_ARITHMETIC=f32 runs every product on v_mfma_f32_32x32x2_f32 (the arithmetic of rounds 1-5): the fp32_mfma_instruction_path leg of this line"}


def eval_knn_leg(device, n=50000, d=128, k=20, reps=10):
    """The reference's kNN evaluation (utils/eval_utils.py:13-21: compute_neighbor_accuracy, k + 1 exact inner-product hits, best dropped) at CIFAR-10's train-set
    size on projected features of BASELINE's width.  Shipped: ONE fused launch (csrc/evalknn.hip knn_fused_k: the Gram product Z Z^T on the bf16x3 arithmetic with a
    streaming top-21 per query on its accumulators - S is never written) + a merge of the column parts.  Beside it, in the same run, the round-3..5 form
    (SSV_ARITHMETIC=f32: Gram in row chunks on the fp32-MFMA GEMM kernel, S written and read back by a one-wavefront-per-query selection).  Wall time per call; kernel
    parts from HIP events per launch (the library's profiling scopes)."""
    from ssv_amd import _lib, ops
    g = torch.Generator(device=device).manual_seed(n)
    z = torch.nn.functional.normalize(torch.randn(n, d, device=device, generator=g), dim=1)
    labels = torch.randint(0, 10, (n,), device=device, generator=g, dtype=torch.int32)

    def timed():
        for _ in range(3):                                    # the first calls of a form run below the clock the following ones hold
            count = ops.knn_label_agreement(z, labels, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            count = ops.knn_label_agreement(z, labels, k)
        ms = (time.perf_counter() - t0) / reps * 1e3
        _lib.prof_enable(True)
        _lib.prof_reset()
        ops.knn_label_agreement(z, labels, k)
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(False)
        return count, ms, prof

    gflop = 2.0 * n * n * d / 1e9
    count, ms, prof = timed()
    fused = ops.ARITHMETIC == "bf16x3"
    kern_ms = prof["misc"][0] + prof["conv_fwd"][0]
    out = {"workload": f"compute_neighbor_accuracy on {n} x {d} unit features, k = {k} (CIFAR-10 train set, proj_dim 128)", "ms_per_call": round(ms, 3),
           "queries_per_sec": round(n / ms * 1e3, 1), "agreement": round(count / (n * k), 5), "arithmetic": ops.ARITHMETIC,
           "form": "fused Gram + top-21 (S never written)" if fused else "Gram on the GEMM kernel, S written, one-wavefront-per-query selection",
           "kernel_ms": round(kern_ms, 3), "algorithmic_gflop": round(gflop, 1), "tflops": round(gflop / kern_ms, 1),
           "roof_tflops": BF16X3_PEAK_TFLOPS if fused else FP32_MFMA_PEAK_TFLOPS, "frac": round(gflop / kern_ms / (BF16X3_PEAK_TFLOPS if fused else FP32_MFMA_PEAK_TFLOPS), 3),
           "timing": "wall clock over %d calls after 3 untimed ones; kernel_ms: HIP events per launch of one more call" % reps}
    if fused:
        with ops.arithmetic("f32"):
            count0, ms0, prof0 = timed()
        gram_ms, sel_ms = prof0["conv_fwd"][0], prof0["misc"][0]
        out["unfused_fp32_path"] = {
            "ms_per_call": round(ms0, 3), "agreement": round(count0 / (n * k), 5),
            "gram": {"ms": round(gram_ms, 3), "tflops": round(gflop / gram_ms, 1), "s_written_gb": round(4.0 * n * n / 1e9, 2)},
            "selection": {"ms": round(sel_ms, 3), "s_read_gb": round(4.0 * n * n / 1e9, 2), "gb_per_s": round(4.0 * n * n / sel_ms / 1e6, 1), "hbm_roof_gb_per_s": 6290.0,
                          "frac": round(4.0 * n * n / sel_ms / 1e6 / 6290.0, 3)}}
        out["speedup_vs_unfused"] = round(ms0 / ms, 2)
        out["count_difference_vs_unfused"] = int(count - count0)
    return out


def fp32_instruction_leg(step, b, world, warmup=2, steps=6):
    """The same step with every product on v_mfma_f32_32x32x2_f32 (ops.arithmetic('f32')), timed in this process after the headline's timed region: either reading of
    `dtype: f32` finds its number in this line."""
    from ssv_amd import ops
    with ops.arithmetic("f32"):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return {"value": round(b * world * steps / dt, 2), "unit": "images/sec", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps, "warmup": warmup,
            "arithmetic": "every product on v_mfma_f32_32x32x2_f32 (SSV_ARITHMETIC=f32), same process, same inputs, after the timed region",
            "roof_tflops": FP32_MFMA_PEAK_TFLOPS}


def conv_macs_resnet50(h, w, proj_dim=128):
    """Algorithmic work per VIEW: MACs of (conv fwd, conv bwd = dgrad + wgrad without the stem's dgrad, projector fwd)
    and the HBM bytes of the conv family when every operand is moved exactly once (fwd + dgrad + wgrad)."""
    macs = []
    strided = 0                               # MACs of the stride-2 layers behind the stem: their dgrad runs on the dgrad kernel
    io = []                                   # (input elements, output elements) per conv, for the algorithmic byte count
    ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    macs.append(ho * wo * 64 * 49 * 3)
    io.append((h * w * 3, ho * wo * 64))
    ho, wo = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    cin = 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            macs.append(ho * wo * planes * cin)                                   # conv1 1x1
            io.append((ho * wo * cin, ho * wo * planes))
            h2, w2 = (ho + 2 - 3) // s + 1, (wo + 2 - 3) // s + 1
            macs.append(h2 * w2 * planes * planes * 9)                            # conv2 3x3 (stride here)
            strided += macs[-1] if s == 2 else 0
            io.append((ho * wo * planes, h2 * w2 * planes))
            macs.append(h2 * w2 * planes * 4 * planes)                            # conv3 1x1
            io.append((h2 * w2 * planes, h2 * w2 * planes * 4))
            if b == 0:
                macs.append(h2 * w2 * planes * 4 * cin)                           # downsample 1x1
                strided += macs[-1] if s == 2 else 0
                io.append((ho * wo * cin, h2 * w2 * planes * 4))
            cin, ho, wo = planes * 4, h2, w2
    fwd = sum(macs)
    bwd = 2 * fwd - macs[0]
    bytes_fwd = 4 * sum(i + o for i, o in io)                        # every operand moved exactly once
    bytes_bwd = 2 * bytes_fwd - 4 * sum(io[0])                       # dgrad + wgrad, no stem dgrad
    return {"fwd": fwd, "bwd": bwd, "bytes_fwd": bytes_fwd, "bytes_bwd": bytes_bwd, "dgrad_s2": strided, "stem": macs[0]}


def step_work(algo, h, w, batch):
    """Algorithmic work of ONE step on one GPU for everything that runs on the conv implicit-GEMM kernels (encoder convs,
    the heads' Linear layers as 1x1 convs, Barlow's three B x D x D GEMMs): (FLOP, HBM bytes of the encoder convs)."""
    c = conv_macs_resnet50(h, w)
    train_views, fwd_only_views = 2, (2 if algo == "byol" else 0)
    if algo == "simclr":
        head_train, head_fwd, loss_macs = 2048 * 2048 + 2048 * 128, 0, 0
    elif algo == "byol":                                             # projector d->d->D and predictor D->D->D online; projector only on the target
        head_train, head_fwd, loss_macs = 2048 * 2048 + 2048 * 128 + 2 * 128 * 128, 2048 * 2048 + 2048 * 128, 0
    else:                                                            # barlow: 2048->4096->4096->4096, C = zi^T zj and the two dz GEMMs once per step
        head_train, head_fwd, loss_macs = 2048 * 4096 + 2 * 4096 * 4096, 0, 3 * 4096 * 4096
    macs_per_sample = train_views * (c["fwd"] + c["bwd"] + 3 * head_train) + fwd_only_views * (c["fwd"] + head_fwd) + loss_macs
    bytes_per_sample = train_views * (c["bytes_fwd"] + c["bytes_bwd"]) + fwd_only_views * c["bytes_fwd"]
    # which kernel runs what: stride-1 dgrad (every layer but the seven stride-2 ones) and the heads' dgrad run on the FORWARD kernel
    dgrad_all = c["fwd"] - c["stem"]
    per_kernel = {"conv_fwd": train_views * (c["fwd"] + dgrad_all - c["dgrad_s2"] + 2 * head_train) + fwd_only_views * (c["fwd"] + head_fwd) + 2 * loss_macs // 3,
                  "conv_dgrad": train_views * c["dgrad_s2"],
                  "conv_wgrad": train_views * (c["fwd"] + head_train) + loss_macs // 3}
    assert sum(per_kernel.values()) == macs_per_sample
    KERNEL_WORK.clear()
    KERNEL_WORK.update({k: 2.0 * v * batch for k, v in per_kernel.items()})
    return 2.0 * macs_per_sample * batch, bytes_per_sample * batch


KERNEL_WORK = {}          # algorithmic FLOP per step of each conv kernel class, filled by step_work()


ALGOS = {"simclr": ("ssv_amd.models.simclr", "SimCLR"), "byol": ("ssv_amd.models.byol", "BYOL"), "barlow": ("ssv_amd.models.barlow", "BarlowTwins"),
         "dino": ("ssv_amd.models.dino", "DINO")}
VITS16 = {"hidden_dim": 384, "embedding_dim": 192, "intermediate_dim": 1536, "num_attention_heads": 6, "patch_size": 16,
          "num_local_patches": 36, "num_global_patches": 196, "num_encoder_layers": 12}          # ViT-S/16 in the reference's encoder vocabulary
DINO_CROPS = {"num_global_views": 2, "num_local_views": 8, "global_size": [224, 224], "local_size": [96, 96], "scale_threshold": 0.3}
BENCH_CFG = {   # the reference configs' hyper-parameters (configs/{simclr,byol,barlow}.yaml) with the std-stem encoder for 224x224
    "simclr": {"proj_dim": 128, "loss_fn": {"normalize": True, "temperature": 0.5}, "optimizer": {"name": "sgd", "lr": 2.0, "weight_decay": 1e-4}},
    "byol": {"proj_dim": 128, "tau": 0.996, "optimizer": {"name": "sgd", "lr": 0.2, "weight_decay": 1e-4}},
    "barlow": {"proj_dim": 4096, "loss_fn": {"normalize": True, "off_diagonal_weight": 0.005}, "optimizer": {"name": "sgd", "lr": 0.2, "weight_decay": 1.5e-6}},
    "dino": {"encoder": VITS16, "proj_head": {"hidden_dim": 512, "proj_dim": 1024}, "gradient_clip": 3.0,
             "optimizer": {"name": "adamw", "lr": 5e-4, "amsgrad": False, "epsilon": 1e-6, "weight_decay": 0.04}},
}


def build(device, algo, steps_per_epoch=1000, lr_scale=1.0, arch="resnet50", reduce_bottom_conv=False):
    """The package's own trainer (ssv_amd.models.<algo>), constructed the way its __init__ does minus dataloaders, output
    directory and wandb; bench steps call its train_step(batch) - the drop-in surface - not a copy of it.  The returned step
    function carries the trainer as ``step.trainer``.  ``lr_scale`` scales the config's learning rate (the parity gate)."""
    import importlib
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import train_utils
    mod, name = ALGOS[algo]
    cls = getattr(importlib.import_module(mod), name)
    t = object.__new__(cls)
    t.config = {"epochs": 1000, "encoder": {"reduce_bottom_conv": reduce_bottom_conv}, "scheduler": {"name": "cosine", "warmup_epochs": 10}, **BENCH_CFG[algo]}
    t.config["optimizer"] = dict(t.config["optimizer"], lr=t.config["optimizer"]["lr"] * lr_scale)
    t.device, t.train_loader = device, [None] * steps_per_epoch
    torch.manual_seed(420)                                     # identical weights on every rank
    t._build("vit" if algo == "dino" else arch)
    t.scheduler, t.warmup_epochs = train_utils.get_scheduler({**t.config["scheduler"], "epochs": 1000}, optimizer=t.optim)   # lr seeded to lr/10
    hdist.attach_grad_sync(t.optim, t._sync_modules())
    state = {"i": 0}

    via_step = os.environ.get("SSV_BENCH_VIA_STEP", "0") == "1"      # diagnostic: the trainer's step() (= the step graph where SSV_STEP_GRAPH allows it) instead of train_step()

    def step(batch):
        loss = (t.step(batch) if via_step else t.train_step(batch))["loss"]
        t._after_step(state["i"])                                # BYOL: tau schedule + EMA of the target, as in the train loop
        state["i"] += 1
        return loss
    step.trainer = t
    return step, sum(p.numel() for p in t.optim.arena.params)


def dino_work(batch):
    """Algorithmic work of one DINO ViT-S/16 multi-crop step on one GPU: (GEMM FLOP of the Linear layers, attention FLOP).
    Per sample the student sees 2 copies x (2 global 197-token + 8 local 37-token) crops forward+backward, the teacher the
    4 global crops forward only.  Attention counts QK^T and PV forward and the four products of the backward (no recompute)."""
    e, head = VITS16, BENCH_CFG["dino"]["proj_head"]
    hid, inter, layers = e["hidden_dim"], e["intermediate_dim"], e["num_encoder_layers"]
    per_token = layers * (3 * hid * hid + 2 * hid * inter) + (3 * e["patch_size"] ** 2 + e["embedding_dim"]) * hid
    per_image_head = hid * head["hidden_dim"] + 2 * head["hidden_dim"] ** 2 + head["hidden_dim"] * head["proj_dim"]
    tg, tl = e["num_global_patches"] + 1, e["num_local_patches"] + 1
    ng, nl = 2 * DINO_CROPS["num_global_views"], 2 * DINO_CROPS["num_local_views"]
    student_tokens, teacher_tokens = ng * tg + nl * tl, ng * tg
    gemm_macs = 3 * (student_tokens * per_token + (ng + nl) * per_image_head) + teacher_tokens * per_token + ng * per_image_head
    attn = lambda t: layers * t * t * hid                       # MACs of ONE T x T x hidden product over all heads
    attn_macs = 6 * (ng * attn(tg) + nl * attn(tl)) + 2 * ng * attn(tg)
    # HBM bytes of the encoder GEMMs when every operand moves once: per token and layer, forward = q/k/v (in 384, out 1152),
    # fc1 (in 384, out 1536), fc2 (in 1536, residual 384, out 384); dgrad and wgrad each move about as much again
    per_token_fwd = 4 * (layers * (2 * hid + 3 * hid + 2 * inter + 2 * hid) + (3 * e["patch_size"] ** 2 + e["embedding_dim"]) + hid)
    gemm_bytes = (3 * student_tokens + teacher_tokens) * per_token_fwd
    return 2.0 * gemm_macs * batch, 2.0 * attn_macs * batch, gemm_bytes * batch


AUG_CFG = {"color_jitter": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4, "hue": 0.1, "apply_prob": 0.8},
           "random_gray": {"p": 0.2}, "random_resized_crop": {"size": [224, 224], "scale": [0.2, 1.0]}, "random_flip": None,
           "to_tensor": None, "normalize": {"mean": [0.485, 0.456, 0.406], "std": [0.229, 0.224, 0.225]}}


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# The parity gate trains at a fraction of the config's learning rate (the gate's own statement, DESIGN 2: ResNet-50 at batch 32 is ill-conditioned at ANY learning rate -
# the fp32 CPU oracle is 1e-3 .. 1e-2 from its own fp64 twin after one update - so FREE-RUNNING steps >= 1 are held to the fp64 envelope of the CPU path, not to a
# fixed 1e-4; the per-step 1e-4 statement is the teacher-forced one).  Barlow Twins' gradient is ~300x its loss: at config / 100 its trajectory is chaotic for every
# evaluation (the CPU oracle ends 13 % from its own fp64 twin after three updates, round 4), so its gate uses config / 10^4, the rate DESIGN 2 measured it tame at.
GATE_LR_SCALES = {"simclr": 0.01, "byol": 0.01, "barlow": 1e-4}


def cpu_baseline(views, steps, algo="simclr", lr_scale=None, fp64=True):
    """The oracle (CPU restatement of the reference step, pinned to reference fixtures) on this box's host cores, on the SAME augmented
    views the GPU path is given: (v1, v2) fp32 [B,3,S,S] CPU tensors.  1 warm-up + `steps` timed fp32 steps (the state every
    step starts from is kept, outside the timed intervals, for the teacher-forced gate); then, untimed, an fp64 twin of the oracle (same
    initial weights) runs the same steps: the centre the free-running gate measures both fp32 paths against."""
    import oracle
    lr_scale = GATE_LR_SCALES[algo] if lr_scale is None else lr_scale
    host = os.cpu_count() or 1
    # SURVEY 8d asks for all host cores; on the 256-thread GPU boxes (2 x EPYC 9575F) the ATen / oneDNN step is pathological at 256 threads
    # (round 2 measured ~320 s for ONE batch-32 step there against 3.5 s at 32 threads; that log was not kept).  Round 6: the thread count is SWEPT - one
    # warm-up + one timed step of a scratch oracle at 32, 64 and 128 threads (those the host has) - and the trajectory below runs at the fastest; the sweep,
    # host_cpus and the CPU model are reported next to the number.
    v1, v2 = views
    batch, size = v1.shape[0], v1.shape[-1]
    base = BENCH_CFG[algo]["optimizer"]
    lr = 1e-12 + base["lr"] * lr_scale / 10                    # get_scheduler's warm-up seeding (utils/train_utils.py:31-33), as the trainer
    if algo == "byol":
        make = lambda: oracle.BYOLOracle("resnet50", False, 128, lr=lr, weight_decay=base["weight_decay"], max_steps=1000 * 1000)
    elif algo == "barlow":
        make = lambda: oracle.BarlowOracle("resnet50", False, 4096, lr=lr, weight_decay=base["weight_decay"], normalize=True)
    else:
        make = lambda: oracle.SimCLROracle("resnet50", False, 128, lr=lr, weight_decay=base["weight_decay"])
    step_of = lambda mm, a, b_: (lambda s: mm.train_step(a, b_, step=s)) if algo == "byol" else (lambda s: mm.train_step(a, b_, **({"return_z": True} if s == 0 else {})))
    sweep = {}
    for nt in sorted({min(host, c) for c in (32, 64, 128)}):
        torch.set_num_threads(nt)
        scratch = make()
        probe = step_of(scratch, v1, v2)
        probe(0)
        t0 = time.perf_counter()
        probe(1)
        sweep[nt] = time.perf_counter() - t0
        del scratch, probe
    torch.set_num_threads(min(sweep, key=sweep.get))
    m = make()
    run = step_of(m, v1, v2)
    first = run(0)                                             # warm-up step = step 0 of the gate
    losses, states, dt = [first["loss"]], [None], 0.0
    for s in range(1, steps + 1):
        states.append(oracle.snapshot(m))                      # what step s starts from (untimed)
        t0 = time.perf_counter()
        losses.append(run(s)["loss"])
        dt += time.perf_counter() - t0
    dt /= steps
    del m
    first64, losses64 = {}, None
    if fp64:
        m64 = oracle.twin64(make)
        run64 = step_of(m64, v1.double(), v2.double())
        first64 = run64(0)
        losses64 = [first64["loss"]] + [run64(s)["loss"] for s in range(1, steps + 1)]
        del m64
    out = {"value": round(batch / dt, 3), "unit": "images/sec", "cores": torch.get_num_threads(), "host_cpus": host, "cpu_model": _cpu_model(), "kind": "port",
           "thread_sweep_images_per_sec": {str(k): round(batch / v, 3) for k, v in sorted(sweep.items())},
           "sample": f"{steps} timed steps (1 warm-up) of the same {algo} ResNet-50 {size}x{size} step at batch {batch} on the GPU path's own augmented views, "
                     f"torch fp32 CPU, lr = config / {round(1 / lr_scale)}"}
    return out, losses, losses64, first.get("z_1"), first64.get("z_1"), states


def _load_cpu_state(t, snap, step, algo):
    """Teacher forcing (checker plumbing): weights + Nesterov momentum (+ BYOL's target weights) of the CPU trajectory -> the HIP trainer,
    which then evaluates step `step` from exactly the state the CPU oracle evaluated it from."""
    from ssv_amd import ops
    from ssv_amd.utils.train_utils import ParamArena
    arena = t.optim.arena
    assert len(arena.params) == len(snap["params"])
    with torch.no_grad():
        for p, off, src, buf in zip(arena.params, arena.offsets, snap["params"], snap["bufs"]):
            assert tuple(p.shape) == tuple(src.shape)
            p.data.copy_(src.to(p.device))
            mv = ParamArena._view(t.optim.momentum_buffer, p, off)
            mv.zero_() if buf is None else mv.copy_(buf.to(p.device))
        if algo == "byol":
            for p, src in zip(t._target_arena.params, snap["target"]):
                p.data.copy_(src.to(p.device))
    t.optim._steps = step
    ops.invalidate_weight_caches()                                  # parameters were overwritten in place


def _dino_gate_batch(batch):
    g = torch.Generator().manual_seed(7)
    mk = lambda v, sz: torch.randn(batch, v, 3, sz, sz, generator=g)
    return {"global_1": mk(2, 224), "global_2": mk(2, 224), "local_1": mk(8, 96), "local_2": mk(8, 96)}


def cpu_baseline_dino(batch=2, steps=6):
    """The DINO oracle (oracle/vit.py: models/dino.py:143-169 restated, pinned by tests/golden/dino_level.npz) on the host cores: 1 warm-up +
    `steps` timed steps on one seeded multi-crop batch.  Returns the baseline record and every step's loss (the parity gate's reference)."""
    from oracle import vit as ovit
    torch.set_num_threads(min(os.cpu_count() or 1, 32))       # batch 2: more threads than work items only adds overhead
    m = ovit.DinoOracle(VITS16, BENCH_CFG["dino"]["proj_head"], lr=5e-4)
    crops = _dino_gate_batch(batch)
    args = (crops["global_1"], crops["global_2"], crops["local_1"], crops["local_2"])
    losses = [m.train_step(*args)["loss"]]                     # warm-up = step 0 of the gate
    t0 = time.perf_counter()
    for _ in range(steps):
        losses.append(m.train_step(*args)["loss"])
    dt = (time.perf_counter() - t0) / steps
    base = {"value": round(batch / dt, 3), "unit": "images/sec", "cores": torch.get_num_threads(), "host_cpus": os.cpu_count(), "cpu_model": _cpu_model(), "kind": "port",
            "sample": f"{steps} timed step (1 warm-up) of the same DINO ViT-S/16 multi-crop step at batch {batch}, torch fp32 CPU"}
    return base, losses


def parity_gate_dino(device, cpu_losses, batch=2, steps=3):
    """BASELINE config 5 in the driver-timed line: a fresh HIP DINO trainer (ViT-S/16, the bench's own configuration and learning rate) and the
    CPU oracle run the same `steps` free-running training steps - student + teacher forward, DinoLoss, clamp, AdamW, centre EMA
    (models/dino.py:143-169) - on the same seeded 2 x (2 x 224 + 8 x 96) crops per sample.  No BatchNorm / ReLU on this path, so the
    north-star's per-step bar applies to the free-running trajectory as it stands: every step's loss within 1e-4 relative."""
    hip_step, _ = build(device, "dino")
    crops = _dino_gate_batch(batch)
    hip = [hip_step(crops) for _ in range(steps)]
    torch.cuda.synchronize()
    del hip_step
    torch.cuda.empty_cache()
    rel = [abs(h - c) / abs(c) for h, c in zip(hip, cpu_losses[:steps])]
    return {"workload": f"DINO ViT-S/16, batch {batch}, 2 copies x (2 global 224 + 8 local 96) seeded normal crops, config lr, {steps} free-running steps on that batch",
            "loss_hip": [round(x, 7) for x in hip], "loss_cpu": [round(x, 7) for x in cpu_losses[:steps]],
            "loss_rel_err": [float(f"{x:.2e}") for x in rel],
            "bar": {"loss_every_step": "1e-4 relative to the fp32 CPU oracle on every step (north-star), free-running"},
            "pass": bool(max(rel) <= 1e-4)}


def parity_gate_and_cpu_baseline(device, algo, tf, source, sample_ids, rows, batch=32, steps=3, fp64=True):
    """SURVEY 8d "parity gates (same run)": the CPU oracle and a fresh HIP trainer run the same `steps`+1 training steps on the same
    `batch` augmented views (the first rows of the bench's own source images).  Two statements:
      * teacher-forced (the north-star's bar, per step): before every step the HIP trainer is given the CPU trajectory's state
        (weights, momentum), so each step is the same pure function on both sides - per-step loss within 1e-4 relative on EVERY step;
      * free-running: the HIP trainer carries its own state - step 0 within 1e-4, later steps inside the fp64 envelope of the CPU path;
    plus the step-0 projected features.  The CPU side of it IS the cpu_baseline timing.
    The HIP trainer of the gate runs under ops.large_batch_dispatch: the Winograd forms' tile-count floors are lifted, so the batch-32 gate
    takes the kernel selection of the timed batch-512 step (F(4x4) on the 14x14 data gradients and the 7x7 layers too); `dispatch` in the
    result counts the launches per form.  ``fp64`` False (the short gates of `other_configs`): no fp64 twin, no free-running envelope -
    step 0 and the teacher-forced steps only."""
    from ssv_amd import ops
    b = min(batch, source.shape[0])
    views = tf.apply(source, rows[:b], tf.draw(source, sample_ids[:b], 0))
    v1, v2 = views[0], views[1]                              # channels_last memory, as the timed steps get them
    base, cpu_losses, f64_losses, z_cpu, z64, states = cpu_baseline((v1.cpu().contiguous(), v2.cpu().contiguous()), steps, algo, fp64=fp64)
    with ops.large_batch_dispatch() as disp:
        hip_step, _ = build(device, algo, lr_scale=GATE_LR_SCALES[algo])
        captured = {}
        t = hip_step.trainer
        if algo in ("simclr", "barlow"):
            inner = t.loss_fn

            def spy(z1, z2):
                captured.setdefault("z_1", z1.detach().float().cpu())
                return inner(z1, z2)
            t.loss_fn = spy
        hip_losses = [hip_step({"aug_1": v1, "aug_2": v2}) for _ in range(steps + 1)]
        torch.cuda.synchronize()
        # teacher-forced: step 0 starts from the common initialisation on both sides (the run above); steps >= 1 from the CPU trajectory's state
        forced = [hip_losses[0]]
        for s_ in range(1, steps + 1):
            _load_cpu_state(t, states[s_], s_, algo)
            forced.append(t.train_step({"aug_1": v1, "aug_2": v2})["loss"])
            t._after_step(s_)
        torch.cuda.synchronize()
        dispatch = {k: round(v / (2 * steps + 1), 1) for k, v in sorted(disp.log.items())}   # launches per step (2 * steps + 1 steps ran)
    del hip_step, t, states
    torch.cuda.empty_cache()
    rel = [abs(h - c) / abs(c) for h, c in zip(hip_losses, cpu_losses)]
    rel_forced = [abs(h - c) / abs(c) for h, c in zip(forced, cpu_losses)]
    sci = lambda xs: [float(f"{x:.2e}") for x in xs]
    if not fp64:
        gate = {"workload": f"{algo} ResNet-50 {v1.shape[-1]}x{v1.shape[-1]}, batch {b}, the bench's own augmented views, lr = config / {round(1 / GATE_LR_SCALES[algo])}, "
                            f"step 0 + {steps} teacher-forced step(s) on that batch",
                "loss_hip_teacher_forced": [round(x, 7) for x in forced], "loss_cpu": [round(x, 7) for x in cpu_losses],
                "loss_rel_err_teacher_forced": sci(rel_forced), "teacher_forced_pass": bool(max(rel_forced) <= 1e-4),
                "dispatch": {"rule": "kernel selection of the batch-512 step (ops.large_batch_dispatch)", "winograd_launches_per_step": dispatch},
                "bar": {"loss_teacher_forced": "1e-4 relative to the fp32 CPU oracle on every step, each step evaluated from the CPU trajectory's own state"}}
        gate["pass"] = bool(rel[0] <= 1e-4 and gate["teacher_forced_pass"])
        return gate, base
    d_hip = [abs(h - f) / abs(f) for h, f in zip(hip_losses, f64_losses)]
    d_cpu = [abs(c - f) / abs(f) for c, f in zip(cpu_losses, f64_losses)]
    gate = {"workload": f"{algo} ResNet-50 {v1.shape[-1]}x{v1.shape[-1]}, batch {b}, the bench's own augmented views, lr = config / {round(1 / GATE_LR_SCALES[algo])}, {steps + 1} steps on that batch",
            "loss_hip_teacher_forced": [round(x, 7) for x in forced], "loss_cpu": [round(x, 7) for x in cpu_losses],
            "loss_rel_err_teacher_forced": sci(rel_forced),
            "teacher_forced_pass": bool(max(rel_forced) <= 1e-4),
            "loss_hip": [round(x, 7) for x in hip_losses], "loss_cpu_fp64": [round(x, 7) for x in f64_losses],
            "loss_rel_err": sci(rel), "loss_rel_err_hip_vs_fp64": sci(d_hip), "loss_rel_err_cpu32_vs_fp64": sci(d_cpu),
            "dispatch": {"rule": "kernel selection of the batch-512 step (ops.large_batch_dispatch: the Winograd forms' tile-count floors lifted for the gate trainer)",
                         "winograd_launches_per_step": dispatch},
            "bar": {"loss_teacher_forced": "1e-4 relative to the fp32 CPU oracle on EVERY step (north-star), each step evaluated from the CPU trajectory's "
                                           "own weights and momentum - the per-step statement",
                    "loss_step0": "1e-4 relative to the fp32 CPU oracle (north-star)",
                    "loss_every_step": "free-running (loss_rel_err): no further from the fp64 twin of the oracle than 3x the furthest the fp32 CPU oracle gets from it on this "
                                       "trajectory, + 1e-4: after one update two fp32 evaluations of this network at batch 32 are 1e-3 .. 1e-2 apart (the CPU oracle "
                                       "against its own fp64 twin: loss_rel_err_cpu32_vs_fp64), so a fixed 1e-4 on a FREE-RUNNING trajectory is not a well-posed bar "
                                       "beyond step 0 (DEVIATION from the north-star's wording for this field only; DESIGN 2, tests/test_gpu_r50_parity.py)",
                    "z_abs_step0": "1e-4, or no further from the fp64 evaluation than 3x the fp32 CPU path is (DEVIATION: the CPU path itself is "
                                   "3-4e-4 from fp64 on this network)"}}
    ok = rel[0] <= 1e-4 and gate["teacher_forced_pass"]
    # steps >= 1: the distance of ONE fp32 evaluation to fp64 at one step is a draw of a chaotic quantity (it can be 5e-4 on one step and 9e-3 on
    # the next); the yardstick is the size class the CPU path shows over the whole trajectory
    worst = max(d_cpu)
    steps_ok = [bool(dh <= (3 * d_cpu[0] + 1e-4 if i == 0 else 3 * worst + 1e-4)) for i, dh in enumerate(d_hip)]
    gate["steps_pass"] = steps_ok
    ok = ok and all(steps_ok)
    if z_cpu is not None and "z_1" in captured:
        dz = float((captured["z_1"] - z_cpu).abs().max())
        gate["z_max_abs_err_step0"] = float(f"{dz:.2e}")
        if z64 is not None:
            e_hip = float((captured["z_1"].double() - z64).abs().max())
            e_cpu = float((z_cpu.double() - z64).abs().max())
            gate["z_err_vs_fp64"] = {"hip": float(f"{e_hip:.2e}"), "cpu_fp32": float(f"{e_cpu:.2e}")}
            ok = ok and (e_hip <= 1e-4 or e_hip <= 3 * e_cpu + 1e-5)
        else:
            ok = ok and dz <= 1e-4
    if algo == "barlow":
        gate["update_at_config_lr"] = update_check(device, algo, v1, v2)
        ok = ok and gate["update_at_config_lr"]["pass"]
    gate["pass"] = bool(ok)
    return gate, base


def update_check(device, algo, v1, v2):
    """The UPDATE path at the config's own learning rate, gated apart from the trajectory (Barlow Twins' loss gate runs at config lr / 10^4, where three steps
    barely move the weights): ONE step from the common initialisation on both sides - CPU oracle and HIP trainer, config lr, weight decay, Nesterov
    momentum (first step: buf = g) - and the weight DELTA compared per tensor.  A delta is lr * (gradient + decay): its error is the gradient's, i.e.
    ReLU-flip sized (1e-2 .. 3e-2 per tensor for ResNet-50 at batch 32 and the config's learning rate, measured) - the bar is that size class, median and worst; an optimizer that applied the wrong
    learning rate, sign, decay or momentum rule would be O(1) off."""
    import oracle
    base = BENCH_CFG[algo]["optimizer"]
    lr = 1e-12 + base["lr"] / 10
    make = {"byol": lambda: oracle.BYOLOracle("resnet50", False, 128, lr=lr, weight_decay=base["weight_decay"], max_steps=1000 * 1000),
            "barlow": lambda: oracle.BarlowOracle("resnet50", False, 4096, lr=lr, weight_decay=base["weight_decay"], normalize=True),
            "simclr": lambda: oracle.SimCLROracle("resnet50", False, 128, lr=lr, weight_decay=base["weight_decay"])}[algo]
    m = make()
    before = oracle.snapshot(m)["params"]
    m.train_step(v1.cpu().contiguous(), v2.cpu().contiguous(), **({"step": 0} if algo == "byol" else {}))
    after = oracle.snapshot(m)["params"]
    del m
    hip_step, _ = build(device, algo)
    arena = hip_step.trainer.optim.arena
    start = [p.detach().float().cpu().clone() for p in arena.params]
    hip_step({"aug_1": v1, "aug_2": v2})
    torch.cuda.synchronize()
    errs, detail = [], []
    largest = max(float((a0 - b0).double().norm()) for b0, a0 in zip(before, after))
    for i, (p, s0, b0, a0) in enumerate(zip(arena.params, start, before, after)):
        d_cpu = (a0 - b0).double()
        if float(d_cpu.norm()) <= 1e-6 * largest:                        # a delta that is nothing but lr * decay * p plus the rounding noise of an analytically zero
            continue                                                     # gradient (a Linear bias in front of a BatchNorm): six orders below the step's deltas
        d_hip = (p.detach().float().cpu() - s0).double()
        errs.append(float((d_hip - d_cpu).norm() / d_cpu.norm()))
        detail.append((errs[-1], i, tuple(p.shape), float(d_cpu.norm()), float(b0.double().norm())))
    del hip_step
    torch.cuda.empty_cache()
    errs.sort()
    detail.sort(reverse=True)
    med, worst = errs[len(errs) // 2], errs[-1]
    return {"workload": f"{algo}: one step at the config's learning rate (lr {lr:.3g}) from the common initialisation, weight delta per tensor, relative l2 vs the CPU oracle",
            "tensors": len(errs), "delta_rel_l2_median": float(f"{med:.2e}"), "delta_rel_l2_worst": float(f"{worst:.2e}"),
            "worst_tensors": [{"rel_l2": float(f"{e:.2e}"), "index": i, "shape": list(sh), "delta_norm": float(f"{dn:.2e}"), "param_norm": float(f"{pn:.2e}")} for e, i, sh, dn, pn in detail[:4]],
            "bar": "median <= 5e-2 and worst <= 0.3 (ReLU-flip size of a batch-32 gradient of this network: 2-3e-2 per tensor; a wrong update rule is O(1))",
            "pass": bool(med <= 5e-2 and worst <= 0.3)}


def read_committed_counters(profiles_dir, fname):
    """A counter file committed under profiles/ and the build it says it was measured on: (data, src_sha16 | None, path relative to the repo) - or
    (None, None, None) when the file does not exist.  JSON files (tools/pmc_traffic.py, tools/pmc_mfma.py) carry `src_sha16`; the per-layer CSV of
    tools/bench_conv.py carries it in its last row (`BUILD src_sha16=... lib_sha16=...`).  The caller replays the data only when src_sha16 equals the
    loaded library's ssv_source_sha16(): counters of another build never reach the bench line."""
    pth = os.path.join(profiles_dir, fname)
    if not os.path.exists(pth):
        return None, None, None
    rel = os.path.relpath(pth, ROOT)
    if pth.endswith(".csv"):
        import csv
        with open(pth, newline="") as fh:
            rows_ = list(csv.DictReader(fh))
        ident = next((r["layer"] for r in rows_ if r["layer"].startswith("BUILD ")), "")
        src = dict(kv.split("=") for kv in ident.split()[1:]).get("src_sha16") if ident else None
        return rows_, src, rel
    with open(pth) as fh:
        data = json.load(fh)
    return data, data.get("src_sha16"), rel


def _config1_views(device, batch):
    from ssv_amd.utils import augmentations
    g = torch.Generator(device=device).manual_seed(421)
    source = torch.randint(0, 256, (batch, 32, 32, 3), generator=g, device=device, dtype=torch.uint8)
    ids = torch.arange(batch, device=device, dtype=torch.int64)
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in AUG_CFG.items()}
    cfg["random_resized_crop"] = {"size": [32, 32], "scale": [0.2, 1.0]}
    cfg["normalize"] = {"mean": [0.4914, 0.4822, 0.4465], "std": [0.2470, 0.2435, 0.2616]}
    tf = augmentations.get_transform(cfg)
    views = tf.apply(source, ids, tf.draw(source, ids, 0))
    return views[0], views[1]


GRAPH_WARM_REPLAYS = 20


def config1_hip(device, batch=64, gpu_steps=50, graph=True):
    """The HIP side of config 1: step-0 loss, `gpu_steps` timed eager steps, then (graph=True) the same trainer's step() replayed as one HIP graph."""
    v1, v2 = _config1_views(device, batch)
    hip_step, _ = build(device, "simclr", arch="resnet18", reduce_bottom_conv=True)
    lr = hip_step.trainer.optim.param_groups[0]["lr"]                  # 2.0 seeded to 1e-12 + 0.2 by get_scheduler, as in the reference
    hip0 = hip_step({"aug_1": v1, "aug_2": v2})
    for _ in range(4):
        hip_step({"aug_1": v1, "aug_2": v2})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(gpu_steps):
        hip_step({"aug_1": v1, "aug_2": v2})
    torch.cuda.synchronize()
    res = {"lr": lr, "hip0": hip0, "eager_dt": (time.perf_counter() - t0) / gpu_steps, "graph_dt": None, "step_graph": None}
    if graph:
        # the same trainer's step through TwoViewTrainer.step: replayed as ONE HIP graph at this size (ssv_amd.graph.StepGraph, SSV_STEP_GRAPH=auto)
        t = hip_step.trainer
        for _ in range(3 + GRAPH_WARM_REPLAYS):                       # two eager steps, the capture, then untimed replays: the first replays after a capture run
            t.step({"aug_1": v1, "aug_2": v2})                        # 5-10 % slower than the steady state a training run sits in (tools/exp/r06_cifar_graph_floors.py)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2 * gpu_steps):
            t.step({"aug_1": v1, "aug_2": v2})
        torch.cuda.synchronize()
        res["graph_dt"] = (time.perf_counter() - t0) / (2 * gpu_steps)
        res["step_graph"] = t._step_graph.describe()
    return res


def config1_line(device, batch=64, cpu_steps=10, gpu_steps=50):
    """BASELINE config 1 / BASELINE.md section 2: the reference's own CPU-runnable case - SimCLR resnet18 (reduce_bottom_conv) on 32 x 32 images at
    batch 64 with configs/simclr.yaml's hyper-parameters (configs/simclr.yaml:38-39) - as `cpu_steps` timed steps of the CPU oracle on this
    box's host cores, next to the same step on the HIP path (same views, fresh trainers on both sides; step-0 loss compared).  The HIP side runs in a CHILD
    process (``bench.py --config1-child``): a fault there (HIP-graph replay is the youngest code of the path) costs this block, never the headline line."""
    import subprocess
    import oracle
    hip, child_error = None, None
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--config1-child", str(batch), str(gpu_steps)], capture_output=True, text=True, timeout=600)
        lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
        if proc.returncode == 0 and lines:
            hip = json.loads(lines[-1])
        else:
            child_error = f"child exit code {proc.returncode}: {proc.stderr.strip().splitlines()[-1] if proc.stderr.strip() else 'no output'}"
    except Exception as exc:
        child_error = f"{type(exc).__name__}: {exc}"
    if hip is None:                                                    # the eager step in this process; the graph figure is then absent, with the reason
        hip = config1_hip(device, batch, gpu_steps, graph=False)
    lr, hip0, eager_dt = hip["lr"], hip["hip0"], hip["eager_dt"]
    v1, v2 = _config1_views(device, batch)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    m = oracle.SimCLROracle("resnet18", True, 128, lr=lr, weight_decay=1e-4)
    c1, c2 = v1.cpu().contiguous(), v2.cpu().contiguous()
    cpu0 = m.train_step(c1, c2)["loss"]                               # warm-up = step 0
    t0 = time.perf_counter()
    for _ in range(cpu_steps):
        m.train_step(c1, c2)
    cpu_dt = (time.perf_counter() - t0) / cpu_steps
    eager = {"value": round(batch / eager_dt, 1), "ms_per_step": round(eager_dt * 1e3, 3),
             "sample": f"{gpu_steps} timed steps (5 warm-up) of train_step() launched kernel by kernel"}
    if hip["graph_dt"] is not None:
        gpu_dt = hip["graph_dt"]
        gpu = {"value": round(batch / gpu_dt, 1), "unit": "images/sec", "ms_per_step": round(gpu_dt * 1e3, 3),
               "sample": f"{2 * gpu_steps} timed steps (after {GRAPH_WARM_REPLAYS} untimed replays) of the HIP trainer's step() on the same views, loss read every step: the step replayed as one HIP graph "
                         "(ssv_amd.graph.StepGraph; ~640 launches whose host enqueue time equals the GPU's work at this size); measured in a child process",
               "step_graph": hip["step_graph"], "eager": eager}
    else:
        gpu = dict(eager, unit="images/sec", step_graph={"error": child_error})
    return {"workload": f"SimCLR resnet18 (reduce_bottom_conv) 32x32, batch {batch}, configs/simclr.yaml hyper-parameters (lr seeded to {lr:.3g}), synthetic uint8 source -> GPU two-view augmentation",
            "cpu": {"value": round(batch / cpu_dt, 1), "unit": "images/sec", "ms_per_step": round(cpu_dt * 1e3, 2), "cores": torch.get_num_threads(), "kind": "port",
                    "sample": f"{cpu_steps} timed steps (1 warm-up) of the oracle, torch fp32 CPU"},
            "gpu": gpu,
            "loss_step0": {"hip": round(hip0, 7), "cpu": round(cpu0, 7), "rel_err": float(f"{abs(hip0 - cpu0) / abs(cpu0):.2e}")}}


def make_step(device, algo, train_step, source, sample_ids, rows, tf, multi_crop):
    """One bench step: fresh augmentation parameters (Philox keyed by GLOBAL sample id and step) -> the views on the input stream ->
    the trainer's own train_step(batch)."""
    from ssv_amd import nn as hnn
    counter = [0]

    def step():
        with hnn.input_stream(device) as ins:                         # as utils/data_utils.GpuTwoViewLoader does: the views are built on their own stream
            if multi_crop is not None:                                # two augmented copies -> 2 x (2 global + 8 local) bicubic crops
                batch = multi_crop(source, rows, counter[0], sample_ids=sample_ids)
            else:
                params = tf.draw(source, sample_ids, counter[0])      # RNG keyed by the GLOBAL sample id
                views = tf.apply(source, rows, params)
                batch = {"aug_1": views[0], "aug_2": views[1]}
            ins.publish(*batch.values())
        counter[0] += 1
        return train_step(batch)
    return step


def time_ntxent(device, nglob, b, d=128, reps=20):
    """The two NT-Xent row kernels alone at ONE RANK's shape - 2b local rows against 2 nglob gathered columns (utils/losses.py:15-46 in the
    row-block form, SURVEY 8e iii) - HIP events on the launch stream, `reps` launches each, with the library's column split and unsplit."""
    from ssv_amd import ops
    g = torch.Generator(device=device).manual_seed(5)
    z = torch.randn(2 * nglob, d, generator=g, device=device)
    z, _ = ops.l2norm_fwd(z, True)
    lse_all = torch.empty(2 * nglob, device=device)
    for r in range(nglob // b):                                   # every row's log-sum-exp (what the second all-gather delivers)
        lse, _ = ops.ntxent_fwd(z, nglob, b, r * b, 2.0)
        lse_all[r * b:(r + 1) * b].copy_(lse[:b])
        lse_all[nglob + r * b:nglob + (r + 1) * b].copy_(lse[b:])
    out = {"rows": 2 * b, "cols": 2 * nglob, "dim": d, "splits": ops.ntxent_splits(nglob, b)}
    for tag, splits in (("", out["splits"]), ("_unsplit", 1)):
        for name, fn in (("fwd", lambda: ops.ntxent_fwd(z, nglob, b, 0, 2.0, splits=splits)),
                         ("bwd", lambda: ops.ntxent_bwd(z, lse_all, nglob, b, 0, 2.0, 2.0 / (2 * nglob), splits=splits))):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[f"{name}_us{tag}"] = round(e0.elapsed_time(e1) / reps * 1e3, 1)
    flop = 2.0 * (2 * b) * (2 * nglob) * d
    out["fwd_tflops"] = round(flop / out["fwd_us"] / 1e6, 1)
    out["bwd_tflops"] = round(2 * flop / out["bwd_us"] / 1e6, 1)      # the Gram tile again + W . Z
    return out


def config3_rank_emulation(device, train_step, step, b, n1_ms, world=8, warmup=2, steps=5):
    """BASELINE config 3 (SimCLR resnet50, global batch 4096 on 8 GPUs) as the step ONE RANK of it executes, measured on the one GPU this run
    has: ssv_amd.distributed.emulate_world(8) - the trainer takes every data-parallel code path (NT-Xent of its 1,024 rows against 8,192
    gathered columns, two all-gathers, per-bucket slab folds and SUM all-reduces launched from the backward pass on the exchange stream)
    with the transport replaced by device copies: the seven peers hold this rank's own shard, for which the emulation is exact
    (tests/test_gpu_config3.py).  What it cannot show is the xGMI time of the collectives (4.2 MB + 36 KB gathered, 112 MB all-reduced
    per step against >= 200 ms of compute)."""
    from ssv_amd import distributed as hdist
    t = train_step.trainer
    mods = t._sync_modules()
    prev = hdist.emulate_world(world, 0)
    try:
        hdist.attach_grad_sync(t.optim, mods)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        buckets = [[n, (hi - lo) * 4] for n, lo, hi in t.optim.grad_sync.buckets]
    finally:
        hdist.detach_grad_sync(t.optim, mods)
        hdist.restore_world(prev)
    return {"emulated_world": world, "rank": 0, "per_rank_batch": b, "global_batch": b * world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms, 3), "images_per_sec_per_rank": round(b / ms * 1e3, 1), "last_loss": loss,
            "n1_ms_per_step": round(n1_ms, 3), "compute_side_scaling_ceiling": round(n1_ms / ms, 4),
            "ceiling_note": "ms_per_step of the single-GPU step / ms_per_step of one rank's step of the 8-GPU job with free transport: the scaling efficiency "
                            "the compute side alone allows (the collectives' xGMI time is NOT in it - no multi-GPU node was available to this build)",
            "ntxent": time_ntxent(device, b * world, b),
            "gradient_buckets": buckets,
            "transport": "emulated (ssv_amd.distributed.emulate_world): all-gather = one device copy of the gathered size with this rank's block in every "
                         "slot, all-reduce(SUM) = x world on the exchange stream; every kernel of the rank's step is the real one"}


def other_config_leg(device, algo, tf, source, sample_ids, rows, cfg, warmup=3, steps=8):
    """BASELINE configs 4 (BYOL resnet50 bs 512 / GPU) and 5 (DINO ViT-S/16 multi-crop bs 128 / GPU) in the driver's default line: a fresh trainer,
    `warmup` + `steps` timed steps of its per-GPU workload, and a short parity gate against the CPU oracle at a small batch."""
    from ssv_amd.utils import augmentations
    b = min(128, source.shape[0]) if algo == "dino" else source.shape[0]
    train_step, nparams = build(device, algo)
    multi_crop = augmentations.MultiCrop({**DINO_CROPS, "train_transforms": cfg}) if algo == "dino" else None
    step = make_step(device, algo, train_step, source[:b], sample_ids[:b], rows[:b], tf, multi_crop)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    # the same trainer as rank 0 of 8 (BASELINE configs 4 / 5 are quoted "on 8xMI355X"): every data-parallel code path, transport replaced by device copies
    from ssv_amd import distributed as hdist
    emu = None
    try:
        t_ = train_step.trainer
        mods = t_._sync_modules()
        prev = hdist.emulate_world(8, 0)
        try:
            hdist.attach_grad_sync(t_.optim, mods)
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(4):
                step()
            torch.cuda.synchronize()
            ems = (time.perf_counter() - t0) / 4 * 1e3
            emu = {"emulated_world": 8, "ms_per_step": round(ems, 3), "compute_side_scaling_ceiling": round(dt * 1e3 / ems, 4),
                   "gradient_buckets": len(t_.optim.grad_sync.buckets), "steps": 4, "warmup": 2}
        finally:
            hdist.detach_grad_sync(t_.optim, mods)
            hdist.restore_world(prev)
    except Exception as exc:
        emu = {"error": f"{type(exc).__name__}: {exc}"}
    del step, train_step
    torch.cuda.empty_cache()
    s = source.shape[1]
    if algo == "dino":
        gemm, attn, _ = dino_work(b)
        flop = gemm + attn
    else:
        flop, _ = step_work(algo, s, s, b)
    out = {"metric": f"images/sec {algo} per-GPU workload of BASELINE config {'5' if algo == 'dino' else '4'}", "value": round(b / dt, 2), "unit": "images/sec",
           "ms_per_step": round(dt * 1e3, 3), "steps": steps, "warmup": warmup, "per_gpu_batch": b, "params": nparams, "last_loss": loss, "dtype": "f32",
           "whole_step_mfma_frac": round(flop / dt / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4), "rank_of_8_emulation": emu}
    if algo == "dino":
        base, cpu_losses = cpu_baseline_dino(batch=2, steps=2)
        gate = parity_gate_dino(device, cpu_losses, batch=2, steps=3)
    else:
        gate, base = parity_gate_and_cpu_baseline(device, algo, tf, source, sample_ids, rows, batch=16, steps=1, fp64=False)
    out.update(parity_gate=gate, cpu_baseline=base)
    out["pass"] = bool(gate["pass"])
    return out


DUMP_PARAMS_MAX = 1 << 23         # float32 elements of the parameter sample: 32 MB, inside the 64 MB a dump may take


def dump_outputs(out_dir, loss, trainer):
    """``--dump-outputs DIR``: what the last timed step handed its caller - the loss (loss.npy, float64 [1]) and the parameters the update
    left (params.npy, float32: the optimizer's flat parameter buffer, every k-th element with the smallest k that keeps it to DUMP_PARAMS_MAX
    elements - a fixed sample, the same on every run with the same arguments)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    flat = trainer.optim.arena.data
    stride = -(-flat.numel() // DUMP_PARAMS_MAX)
    np.save(os.path.join(out_dir, "loss.npy"), np.asarray([loss], dtype=np.float64))
    np.save(os.path.join(out_dir, "params.npy"), flat[::stride].detach().float().cpu().numpy())


def config1_child(argv):
    """``bench.py --config1-child BATCH STEPS``: the HIP side of config_1's block, alone in this process; one JSON line on stdout."""
    from ssv_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench.py --config1-child needs an MI355X")
    _lib.load()
    device = torch.device("cuda", torch.cuda.current_device())
    print(json.dumps(config1_hip(device, int(argv[0]), int(argv[1]))), flush=True)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--config1-child":
        return config1_child(sys.argv[2:4])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (images); default 512, 128 for --algo dino (BASELINE configs)")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--algo", choices=tuple(ALGOS), default="simclr", help="simclr = BASELINE.json's metric; byol = its config 4")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--prof-steps", type=int, default=2, help="extra instrumented steps for the per-kernel-class roofline")
    ap.add_argument("--emulate-world", type=int, default=0, help="W > 1: this ONE process runs the step of rank 0 of a W-rank job "
                    "(ssv_amd.distributed.emulate_world: every data-parallel code path, transport replaced by device copies)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the config3_rank_emulation / other_configs (BYOL, DINO) legs of the default line")
    ap.add_argument("--no-arith-legs", action="store_true", help="skip the arithmetic block and the fp32-instruction leg (profiling runs: only the shipped step's kernels in the trace)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline, after the timed region: roofline, arithmetic and fp32-instruction "
                    "legs, config-3 emulation, collective timing, CPU baseline and parity gates, config 1, kNN and BYOL / DINO legs (the --no-* switches "
                    "and --prof-steps trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's loss and a fixed sample of the parameters it "
                    "left as DIR/{loss,params}.npy (rank 0)")
    args = ap.parse_args()

    from ssv_amd import _lib, distributed as hdist
    rank, world = hdist.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the process group has {world} rank(s): an outer launcher must start exactly --gpus ranks "
                         f"(python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 bench.py --gpus {args.gpus} ...), "
                         f"or run plain `python bench.py --gpus {args.gpus}` and let it start them")
    if not torch.cuda.is_available():
        raise SystemExit(f"bench.py needs an MI355X: no HIP device visible (rank {rank} of {world})")
    device = torch.device("cuda", torch.cuda.current_device())
    _lib.load()
    if args.emulate_world > 1:
        if world != 1:
            raise SystemExit("--emulate-world runs in ONE process (it replaces the process group): use it with --gpus 1")
        hdist.emulate_world(args.emulate_world, 0)                    # before build(): the trainer attaches its gradient buckets

    if args.batch is None:
        args.batch = int(os.environ.get("SSV_BENCH_BATCH", "128" if args.algo == "dino" else "512"))
    b, s = args.batch, args.size
    from ssv_amd import nn as hnn
    train_step, nparams = build(device, args.algo)
    # synthetic uint8 source images [B,S,S,3] ~ U{0..255}, resident in HBM before the timed region; every step draws
    # fresh augmentation parameters (Philox keyed by global sample index and step) and builds the two views on the GPU
    from ssv_amd.utils import augmentations
    g = torch.Generator(device=device).manual_seed(420 + rank)
    source = torch.randint(0, 256, (b, s, s, 3), generator=g, device=device, dtype=torch.uint8)
    sample_ids = torch.arange(rank * b, (rank + 1) * b, device=device, dtype=torch.int64)
    rows = torch.arange(b, device=device, dtype=torch.int64)
    hnn.data_ready(device)                                            # the generated source images: input_stream blocks wait for this event
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in AUG_CFG.items()}
    cfg["random_resized_crop"] = {"size": [s, s], "scale": [0.2, 1.0]}
    tf = augmentations.get_transform(cfg)
    multi_crop = augmentations.MultiCrop({**DINO_CROPS, "train_transforms": cfg}) if args.algo == "dino" else None
    step = make_step(device, args.algo, train_step, source, sample_ids, rows, tf, multi_crop)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    loss = None
    for _ in range(args.warmup):
        loss = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, train_step.trainer)
    dist_info = None
    if world > 1:
        import torch.distributed as dist
        per_rank = [None] * world
        dist.all_gather_object(per_rank, float(dt))
        dt = max(per_rank)                                         # MAX over ranks: the step is as slow as its slowest rank
        comms = None
        if args.full:
            # what the exchange costs: extra steps (after the timed region) with an event pair around every collective, on the stream it runs on
            hdist.comm_timing(True)
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            comms = [None] * world
            dist.all_gather_object(comms, hdist.comm_timing(False) / 2)
        sync = getattr(train_step.trainer.optim, "grad_sync", None)
        props = torch.cuda.get_device_properties(device)
        mine_dev = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "pid": os.getpid(), "device": device.index, "name": props.name,
                    "uuid": str(getattr(props, "uuid", "")), "pci_bus_id": getattr(props, "pci_bus_id", None)}
        devices = [None] * world
        dist.all_gather_object(devices, mine_dev)                  # what every rank really ran on: N distinct devices prove one process per GPU
        dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks_per_gpu": max(1, dist.get_world_size() // max(1, torch.cuda.device_count())),
                     "launched_by": "bench.py (ssv_amd.launch: child torch.distributed.run)" if os.environ.get("SSV_LAUNCHED_BY") else "outer launcher",
                     "devices": devices,
                     "ms_per_step_min_over_ranks": round(min(per_rank) / args.steps * 1e3, 3), "ms_per_step_max_over_ranks": round(max(per_rank) / args.steps * 1e3, 3),
                     "comm_ms_per_step": None if comms is None else round(max(comms), 3),
                     "comm_note": "device time between HIP events around every collective (embedding / LSE all-gathers, per-bucket gradient all-reduces on the "
                                  "exchange stream), max over ranks, 2 extra steps; the bucketed all-reduces overlap the backward pass, so this is not additive to ms_per_step",
                     "gradient_buckets": None if sync is None else [[n, (hi - lo) * 4] for n, lo, hi in sync.buckets]}
        assert dist_info["world_size"] == args.gpus
    ms_per_step = dt / args.steps * 1e3
    images_per_s = b * world * args.steps / dt

    # ---- per-kernel-class timing (HIP events on the launch stream) over extra instrumented steps --------------
    if args.algo == "dino":
        conv_flop_step, attn_flop_step, algo_bytes_step = dino_work(b)
    else:
        conv_flop_step, algo_bytes_step = step_work(args.algo, s, s, b)       # per GPU and step; 2 FLOP/MAC
        attn_flop_step = 0.0
    roof, classes = None, {}
    if args.full and args.prof_steps > 0:
        # per-kernel durations are only meaningful when kernels do not overlap: the instrumented steps run the two
        # views back to back on ONE stream (the timed region above runs them on two streams)
        was_dual = hnn.set_view_streams(False)
        step(); torch.cuda.synchronize()
        _lib.prof_enable(True)
        _lib.prof_reset()
        for _ in range(args.prof_steps):
            step()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(False)
        hnn.set_view_streams(was_dual)
        classes = {k: {"ms_per_step": round(v[0] / args.prof_steps, 3), "launches_per_step": v[1] // args.prof_steps} for k, v in prof.items() if v[1]}
        for k, flop in KERNEL_WORK.items():        # per kernel: algorithmic FLOP / its own summed duration (cross-check with profiles/*kernel_stats*.csv)
            if k in classes and classes[k]["ms_per_step"] > 0:
                classes[k].update(algorithmic_gflop_per_step=round(flop / 1e9, 1), tflops=round(flop / classes[k]["ms_per_step"] / 1e9, 2),
                                  avg_launch_ms=round(classes[k]["ms_per_step"] / classes[k]["launches_per_step"], 4))
        conv_ms = sum(prof[k][0] for k in ("conv_fwd", "conv_dgrad", "conv_wgrad")) / args.prof_steps
        conv_launch = sum(prof[k][1] for k in ("conv_fwd", "conv_dgrad", "conv_wgrad")) // args.prof_steps
        ach = conv_flop_step / (conv_ms * 1e-3) / 1e12
        # counters measured in separate rocprofv3 --pmc runs (they cannot be collected inside this process): replayed from profiles/ ONLY when the file
        # was measured on the build that is loaded now
        my_src, my_lib = _lib.source_sha16(), _lib.lib_sha16()
        stale, used = [], {}

        def committed(fname, kind):
            data, src, rel = read_committed_counters(os.path.join(ROOT, "profiles"), fname)
            if rel is None:
                return None
            if src != my_src:
                stale.append({"file": rel, "measured_on_src_sha16": src})
                return None
            used[kind] = rel
            return data
        traffic, whole_traffic, pmc = None, None, None
        if args.algo in PMC_FILES:       # HBM bytes of the same kernels: rocprofv3 PMC FETCH_SIZE, WRITE_SIZE, corrected as the guide prescribes
            pmc = committed(PMC_FILES[args.algo] % b, "traffic")
            if pmc is not None:
                pmc = pmc["per_step_gb"]
                traffic = round(sum(pmc[k]["fetch"] + pmc[k]["write"] for k in ("conv_fwd", "conv_dgrad", "conv_wgrad") if k in pmc), 1)
                whole_traffic = round(sum(v["fetch"] + v["write"] for v in pmc.values()), 1)
                for k, v in pmc.items():
                    if k in classes:
                        classes[k]["hbm_gb_per_step"] = round(v["fetch"] + v["write"], 1)
        mfma, executed_gflop, family_clock = None, None, None
        if args.algo in PMC_MFMA_FILES:  # matrix-pipe utilisation: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE (tools/pmc_mfma.py)
            mfma = committed(PMC_MFMA_FILES[args.algo] % b, "mfma")
            if mfma is not None:
                for k, v in mfma["per_class"].items():
                    if k in classes and v.get("mfma_busy_frac") is not None:
                        classes[k]["mfma_busy_frac"] = v["mfma_busy_frac"]
                        if v.get("effective_clock_ghz") is not None:
                            classes[k]["effective_clock_ghz"] = v["effective_clock_ghz"]
                executed_gflop = mfma["summary"].get("conv_family_executed_gflop_per_step")
                family_clock = mfma["summary"].get("conv_family_effective_clock_ghz")
                mfma = dict(mfma["summary"], source=used["mfma"])
        # operand streams of the conv family in the variants the step launches (the fused BatchNorm operands - shortcut, BatchNorm input, gate
        # operands, the written activation - are streams of these kernels now): per view from tools/bench_conv.py's per-layer model, x 2 views
        family_gb, family_src, traffic_ratios = None, None, None
        if args.algo == "simclr":
            layer_rows = committed(CONV_LAYER_FILE % b, "layers")
            if layer_rows is not None:
                tot = {r["layer"].split()[1]: 2 * float(r["fwd_GB"]) for r in layer_rows if r["layer"].startswith("TOTAL")}       # per product, two views
                family_gb, family_src = round(sum(tot.values()), 1), used["layers"]
                if pmc is not None:
                    # counted (PMC) next to algorithmic (every operand stream of the launched variant once) per kernel class.  The forward-kernel class also runs the
                    # stride-1 data gradients (forward kernel on the transposed filter) and the Winograd input / output transforms; the data-gradient class the strided
                    # kernel and the gated Winograd output transforms: the two are priced together.  The transformed-domain tensors of the Winograd layers (V, M, the
                    # transformed gradients) are counted bytes that the algorithmic figure does not have - the bytes the 2.25-4x fewer multiplies are bought with.
                    cnt = lambda *ks: sum(pmc[k]["fetch"] + pmc[k]["write"] for k in ks if k in pmc)
                    pairs = {"conv_fwd+conv_dgrad": (cnt("conv_fwd", "conv_dgrad"), tot.get("fwd", 0.0) + tot.get("dgrad", 0.0)), "conv_wgrad": (cnt("conv_wgrad"), tot.get("wgrad", 0.0))}
                    traffic_ratios = {k: {"counted_gb": round(c, 1), "algorithmic_gb": round(a, 1), "ratio": round(c / a, 3) if a else None} for k, (c, a) in pairs.items()}
                    for k in ("bn_fwd", "bn_bwd", "aug", "pool", "optim", "loss", "misc"):
                        if k in pmc:
                            traffic_ratios[k] = {"counted_gb": round(pmc[k]["fetch"] + pmc[k]["write"], 1), "algorithmic_gb": None,
                                                 "note": "streaming passes: every byte counted is a byte the pass exists to move (their algorithmic figure is 0 once fused away)"}
                    traffic_ratios["whole_step"] = {"counted_gb": whole_traffic, "survey_8d_streaming_model_gb": round(1.067 * b, 1), "ratio": round(whole_traffic / (1.067 * b), 3)}
        attn_ms = prof.get("attn", (0.0, 0))[0] / args.prof_steps
        from ssv_amd import ops as _ops
        bf = _ops.ARITHMETIC == "bf16x3"
        peak = BF16X3_PEAK_TFLOPS if bf else FP32_MFMA_PEAK_TFLOPS
        roof = {"bound": "mfma", "kernel": ("implicit-GEMM family running the Linear layers" if args.algo == "dino" else "conv implicit-GEMM family") +
                                           (" (fwd+dgrad+wgrad; fp32 products as 6 bf16 piece products on v_mfma_f32_16x16x32_bf16)" if bf else " (fwd+dgrad+wgrad, fp32 v_mfma_f32_32x32x2_f32)"),
                "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                "peak_is": ("dense bf16 MFMA peak 2,500 TFLOP/s / 6 piece products per fp32 product = 416.7 TFLOP/s of fp32 products" if bf else "fp32 MFMA peak (v_mfma_f32_32x32x2_f32)"),
                "frac_vs_fp32_mfma_roof": round(ach / FP32_MFMA_PEAK_TFLOPS, 4),
                # `frac` / `frac_algorithmic` price the reference's ALGORITHMIC FLOPs (direct convolution); the Winograd layers execute
                # 2.25x fewer multiplies, so the matrix pipe's own utilisation is `executed_frac` = FLOPs the MFMA counters saw / the same family time
                "frac_algorithmic": round(ach / peak, 4),
                "executed_frac": None if executed_gflop is None else round(executed_gflop / conv_ms / peak, 4),
                "executed_gflop_per_step": executed_gflop,
                # the clock the chip held while the family's kernels ran in the counter pass (GRBM_GUI_ACTIVE / 8 XCDs / kernel time: DVFS under the fp32 MFMA
                # load, MI355X_MICROARCH.md); `peak` above is the guide's figure at 2.4 GHz, so executed_frac ~= matrix-pipe busy fraction x clock / 2.4
                "effective_clock_ghz": family_clock,
                "executed_frac_of_peak_at_that_clock": None if (executed_gflop is None or not family_clock) else round(executed_gflop / conv_ms / (peak * family_clock / 2.4), 4),
                "counters_src_sha16": my_src, "counters_lib_sha16": my_lib, "counters_stale": bool(stale), "counters_rejected": stale or None,
                "counters_note": "src_sha16 = the sources the LOADED library was compiled from (ssv_source_sha16; hipcc output is not bit-reproducible, so the file hash "
                                 "lib_sha16 only identifies one build artefact); traffic / mfma_counters / executed_frac / algorithmic_gb_per_step are replayed from "
                                 "profiles/ only when measured on this src_sha16",
                "traffic": traffic, "traffic_unit": "GB of HBM traffic per step for this kernel family (rocprofv3 PMC FETCH_SIZE + WRITE_SIZE, %s)" % (used.get("traffic") or "no PMC pass measured on this build"),
                "algorithmic_gb_per_step": family_gb if family_gb is not None else (None if algo_bytes_step is None else round(algo_bytes_step / 1e9, 1)),
                "algorithmic_gb_note": ("every operand stream of the family's kernels moved once, fused BatchNorm operands included (%s); the transformed-domain "
                                        "tensors of the Winograd layers (V, M, transformed gradients: ~150 GB/step at bs 512 - bytes traded for 2.25x fewer multiplies, "
                                        "DESIGN 4.4) are in `traffic` but NOT in this figure" % family_src) if family_gb is not None
                                       else "conv operands only (x, w, y once per product): the fused BatchNorm streams these kernels also carry are NOT in this figure",
                "conv_operands_only_gb_per_step": None if algo_bytes_step is None else round(algo_bytes_step / 1e9, 1),
                "traffic_ratios": traffic_ratios,
                # whole step: PMC traffic of ALL kernels against SURVEY 8(d)'s streaming model (1.067 GB / sample: 12 fp32 accesses per conv-output element)
                "whole_step_traffic_gb": whole_traffic,
                "whole_step_algorithmic_gb": round(1.067 * b, 1) if args.algo == "simclr" else None,
                "algorithmic_gflop_per_step": round(conv_flop_step / 1e9, 1), "kernel_ms_per_step": round(conv_ms, 3),
                "launches_per_step": int(conv_launch), "avg_launch_ms": round(conv_ms / max(conv_launch, 1), 4),
                "timing": "HIP events per launch over %d extra single-stream steps after the timed region" % args.prof_steps,
                "whole_step_mfma_frac": round(images_per_s / world * (conv_flop_step + attn_flop_step) / b / 1e12 / peak, 4),
                "whole_step_frac_vs_fp32_mfma_roof": round(images_per_s / world * (conv_flop_step + attn_flop_step) / b / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                "mfma_counters": mfma,
                "attention": None if not attn_flop_step else {"algorithmic_gflop_per_step": round(attn_flop_step / 1e9, 1), "kernel_ms_per_step": round(attn_ms, 3),
                                                              "achieved_tflops": round(attn_flop_step / max(attn_ms, 1e-9) / 1e9, 2)},
                "classes": classes}

    # ---- the same step on the fp32 MFMA instruction, and what the shipped arithmetic is (rank 0, one GPU: after the timed region) ----
    fp32_leg, arith = None, None
    if args.full and rank == 0 and world == 1 and not args.emulate_world and not args.no_arith_legs:
        from ssv_amd import ops as _ops
        try:
            arith = arithmetic_block(device)
            if _ops.ARITHMETIC == "bf16x3":
                fp32_leg = fp32_instruction_leg(step, b, world)
        except Exception as exc:
            fp32_leg = {"error": f"{type(exc).__name__}: {exc}"}

    # ---- BASELINE config 3's per-rank step on this one GPU (default SimCLR line only; after the timed region and the instrumented steps) ----
    emu_block = None
    legs = args.full and rank == 0 and world == 1 and args.algo == "simclr" and not args.emulate_world and not args.no_other_configs
    if legs:
        try:
            emu_block = config3_rank_emulation(device, train_step, step, b, ms_per_step)
        except Exception as exc:                                       # a failing extra leg must not take the headline line with it
            emu_block = {"error": f"{type(exc).__name__}: {exc}"}
    emu_self = None
    if args.emulate_world > 1:                                         # --emulate-world W: the whole line IS one rank's step of the W-rank job
        emu_self = {"emulated_world": args.emulate_world, "rank": 0, "global_batch": b * args.emulate_world,
                    "value_is": "images/sec of ONE rank's step (per-rank batch / step time); the W-rank job with free transport would run W x that",
                    "ntxent": time_ntxent(device, b * args.emulate_world, b) if args.full and args.algo == "simclr" else None,
                    "gradient_buckets": [[n, (hi - lo) * 4] for n, lo, hi in train_step.trainer.optim.grad_sync.buckets],
                    "transport": "emulated (ssv_amd.distributed.emulate_world): all-gather = one device copy of the gathered size with this rank's block in "
                                 "every slot, all-reduce(SUM) = x world on the exchange stream; every kernel of the rank's step is the real one"}
        hdist.emulate_world(None)

    label = {"simclr": "SimCLR", "byol": "BYOL", "barlow": "Barlow Twins", "dino": "DINO"}[args.algo]
    loss_desc = {"simclr": "NT-Xent(normalize, T=0.5) over the global batch", "byol": "EMA target encoder (4 encoder passes), pair MSE of unit vectors",
                 "barlow": "cross-correlation loss D=4096 over the global batch",
                 "dino": "multi-crop 2 copies x (2 global 224 + 8 local 96), softmax-centering loss K=1024, AdamW + clamp"}[args.algo]
    net_desc = "ViT-S/16 (reference encoder form)" if args.algo == "dino" else "resnet50 (7x7/2 stem)"
    out = {
        "metric": f"images/sec (whole node) {label} {'ViT-S/16 multi-crop' if args.algo == 'dino' else 'ResNet-50 two-view'} train step", "value": round(images_per_s, 2), "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{label} {net_desc} synthetic 3x{s}x{s}, bs={b}/GPU, global batch {b * world}, "
                               f"{loss_desc}" + ("" if args.algo == "dino" else ", SGD-Nesterov"),
                   "input": f"uint8 [B,{s},{s},3] source resident in HBM -> fused GPU two-view augmentation each step",
                   "per_gpu_batch": b, "global_batch": b * world, "image": [3, s, s], "params": nparams,
                   "parallelism": f"dp{world}" if world > 1 else "single", "view_streams": 2 if hnn.view_streams() else 1, "last_loss": loss,
                   "peak_hbm_gb": round(torch.cuda.max_memory_allocated(device) / 1e9, 1),
                   # every SSV_* variable in the environment: the product's diagnostic switches - {} = the shipped kernel selection
                   "diagnostic_switches": {k: v for k, v in sorted(os.environ.items()) if k.startswith("SSV_")},
                   "library": os.path.relpath(_lib.LIB_PATH, ROOT)},
        "arithmetic": arith,
        "fp32_mfma_instruction_path": fp32_leg,
        "roofline": roof,
        "distributed": dist_info,
    }
    if emu_self is not None:
        out["emulated_world"] = emu_self
    if emu_block is not None:
        out["config3_rank_emulation"] = emu_block
    del step, train_step                                               # the extra legs below build their own trainers
    torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        if args.algo == "dino":
            out["cpu_baseline"], dino_cpu_losses = cpu_baseline_dino()
            out["parity_gate"] = parity_gate_dino(device, dino_cpu_losses)
        else:
            out["parity_gate"], out["cpu_baseline"] = parity_gate_and_cpu_baseline(device, args.algo, tf, source, sample_ids, rows)
            if args.algo == "simclr":
                out["config1"] = config1_line(device)
                try:
                    out["eval_knn"] = eval_knn_leg(device)
                except Exception as exc:
                    out["eval_knn"] = {"error": f"{type(exc).__name__}: {exc}"}
        if legs:                                                       # BASELINE configs 4 and 5, driver-visible: each leg on its own, errors recorded
            out["other_configs"] = {}
            for other in ("byol", "dino"):
                t_leg = time.perf_counter()
                try:
                    out["other_configs"][other] = other_config_leg(device, other, tf, source, sample_ids, rows, cfg)
                except Exception as exc:
                    out["other_configs"][other] = {"error": f"{type(exc).__name__}: {exc}", "pass": False}
                    torch.cuda.empty_cache()
                out["other_configs"][other]["leg_seconds"] = round(time.perf_counter() - t_leg, 1)
    elif rank == 0:
        out["cpu_baseline"], out["parity_gate"] = None, None
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
