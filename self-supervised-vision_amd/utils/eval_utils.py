"""Evaluation helpers.

compute_neighbor_accuracy is the reference's 20-NN label agreement (utils/eval_utils.py:13-21, faiss.IndexFlatIP search) as
one C-ABI call: S = Z Z^T on the fp32-MFMA GEMM kernel, streaming top-(k+1) per query on the GPU (csrc/evalknn.hip) - no faiss,
and `eval_every` costs milliseconds.  linear_evaluation is a small closed loop on frozen features.
kmeans / compute_cluster_accuracy: Lloyd's k-means on the GPU (csrc/kmeans.hip) and the cluster accuracy after Hungarian matching - the
metric the reference's README reports and its code never computes (it has hungarian_match and a faiss.Kmeans run, nothing joins them).
knn_classify: the weighted kNN classifier of InstDisc / MoCo / DINO (test features search the TRAIN bank, the k best neighbours vote with weight
exp(similarity / T); csrc/knnclassify.hip) - top-1 / top-5 accuracy without any training.  The reference has no such metric.
"""
import numpy as np
import torch

from .. import ops


def compute_neighbor_accuracy(fvecs, targets, k=20, device=None):
    """fvecs [n,d] and targets [n]: numpy arrays (what build_features returns) or tensors already on the GPU."""
    z, device = _features_on_device(fvecs, device, "compute_neighbor_accuracy")
    labels = torch.as_tensor(targets).to(device=device, dtype=torch.int32).contiguous()
    n = z.shape[0]
    if labels.shape != (n,):
        raise ValueError(f"expected fvecs [n,d] and targets [n], got {tuple(z.shape)} and {tuple(labels.shape)}")
    k = min(int(k), n - 1)                                          # tiny evaluation sets (synthetic smoke runs)
    return ops.knn_label_agreement(z, labels, k) / float(n * k)


def hungarian_match(preds, targets, preds_k, targets_k):
    from scipy.optimize import linear_sum_assignment
    votes = np.zeros((preds_k, targets_k))
    for c1 in range(preds_k):
        for c2 in range(targets_k):
            votes[c1, c2] = int(((preds == c1) & (targets == c2)).sum())
    rows, cols = linear_sum_assignment(preds.shape[0] - votes)
    return list(zip(rows.tolist(), cols.tolist()))


def _features_on_device(fvecs, device, who):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} runs on the GPU (libssv_hip); no HIP device is visible and there is no CPU fallback")
    device = device or torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(fvecs, dtype=torch.float32).to(device).contiguous()
    if x.dim() != 2:
        raise ValueError(f"{who}: expected fvecs [n,d], got {tuple(x.shape)}")
    return x, device


def kmeans(fvecs, k, niter=25, nredo=1, seed=1234, device=None):
    """Lloyd's k-means on the GPU (ops.kmeans_assign / ops.kmeans_update); the defaults are faiss.Kmeans's (niter 25, nredo 1, seed 1234).
    Returns {"centroids" [k,d] fp32, "labels" [n] int32 (the assignment to the RETURNED centroids), "objective" (its sum of squared distances, a float),
    "objectives" (one float per iteration of the winning run: the objective of the assignment that iteration's update was made from)}, tensors on the device.

    Redo r starts from the rows torch.randperm(n, generator=torch.Generator().manual_seed(seed + r))[:k] and runs exactly ``niter`` iterations (assign, update) - no
    early stop, no host synchronisation inside the loop: the objectives are gathered in a device array and read once per redo.  The run with the lowest FINAL
    objective wins, the lower r on a tie.  Equal inputs give equal bits.

    Where this departs from faiss.Kmeans (the reference's models/deep_cluster.py:100-118):
      * a cluster that loses all its members KEEPS its centroid (faiss splits a large cluster to refill it);
      * the initial centroids are drawn with torch.randperm as above, not with faiss's own generator: the same seed does not give faiss's start;
      * every point takes part in every iteration (faiss subsamples to max_points_per_centroid = 256 points per centroid)."""
    x, device = _features_on_device(fvecs, device, "kmeans")
    n, k, niter, nredo = x.shape[0], int(k), int(niter), int(nredo)
    if not 1 <= k <= n:
        raise ValueError(f"kmeans: need 1 <= k <= n (got k = {k}, n = {n})")
    if niter < 1 or nredo < 1:
        raise ValueError(f"kmeans: niter and nredo must be at least 1 (got {niter}, {nredo})")
    d = x.shape[1]
    if d % 4:
        x = torch.nn.functional.pad(x, (0, 4 - d % 4))            # once, not once per call: zero columns change no distance and stay zero in every mean
    best = None
    for r in range(nredo):
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + r))[:k].to(device)
        centroids = x[rows].contiguous()
        prep = ops.kmeans_prep(x, centroids)
        trace = torch.empty(niter + 1, dtype=torch.float32, device=device)
        ready = False
        for it in range(niter):
            labels, _, counts, objective = ops.kmeans_assign(x, centroids, prep=prep, prep_ready=ready)
            trace[it].copy_(objective)
            ops.kmeans_update(x, labels, counts, centroids, prep=prep)
            ready = True
        labels, _, _, objective = ops.kmeans_assign(x, centroids, prep=prep, prep_ready=True)      # the assignment to the centroids that are returned
        trace[niter].copy_(objective)
        trace = trace.cpu().tolist()                                                                # the one read of this redo
        if best is None or trace[niter] < best["objective"]:
            best = {"centroids": centroids[:, :d].contiguous(), "labels": labels, "objective": trace[niter], "objectives": trace[:niter], "redo": r}
    return best


def cluster_concentration(dist, labels, counts, alpha=10.0, temperature=0.2):
    """PCL's concentration phi [k] (Li et al., ICLR 2021, eq. 12 and the authors' run_kmeans), fp32 on the device, from what ops.kmeans_assign returns: dist [n]
    squared distances, labels [n] int32, counts [k] int32.  Per cluster phi = mean over its members of sqrt(dist) / log(count + alpha); a cluster with at most one
    member takes the largest phi of the others; phi is clipped to its 10th and 90th percentiles (linear interpolation, numpy.percentile's default) and scaled so
    that its mean is ``temperature``.  The sums run in double in a fixed order - members sorted by (label, index), one running sum, differences at the cluster
    boundaries - without atomics: equal inputs give equal bits.  No host synchronisation."""
    if not (dist.is_cuda and labels.is_cuda and counts.is_cuda):
        raise RuntimeError("cluster_concentration runs on the GPU; there is no CPU fallback")
    n, k = dist.numel(), counts.numel()
    if dist.dim() != 1 or labels.shape != (n,) or counts.dim() != 1 or k < 1 or n < 1:
        raise ValueError(f"cluster_concentration: expected dist [n], labels [n] and counts [k], got {tuple(dist.shape)}, {tuple(labels.shape)}, {tuple(counts.shape)}")
    if not (float(alpha) > 1.0 and float(temperature) > 0.0):
        raise ValueError(f"cluster_concentration: need alpha > 1 and temperature > 0 (got {alpha}, {temperature})")
    order = torch.sort(labels.to(torch.int64), stable=True).indices                     # members by (label, index)
    run = torch.cumsum(dist.to(torch.float64).clamp_min(0.0).sqrt()[order], 0)             # one running sum in double
    run = torch.cat([run.new_zeros(1), run])
    cnt = counts.to(torch.int64)
    ends = torch.cumsum(cnt, 0)
    sums = run[ends] - run[ends - cnt]
    cntd = cnt.to(torch.float64)
    phi = sums / cntd.clamp_min(1.0) / torch.log(cntd + float(alpha))
    many = cnt > 1
    top = torch.where(many, phi, phi.new_full((), -1.0)).max()
    top = torch.where(top >= 0, top, top.new_ones(()))                                   # no cluster with two members: every phi is equal
    phi = torch.where(many, phi, top)
    lo, hi = torch.quantile(phi, phi.new_tensor([0.1, 0.9]))
    phi = torch.minimum(torch.maximum(phi, lo), hi)
    return (phi * (float(temperature) / phi.mean())).to(torch.float32)


def compute_cluster_accuracy(fvecs, targets, num_classes=None, niter=25, nredo=1, seed=1234, device=None):
    """Cluster accuracy after Hungarian matching: k-means with k = num_classes (default targets.max() + 1) on the GPU, the cluster x class vote table on the GPU
    (ops.cluster_votes), scipy's linear_sum_assignment(n - votes) as in hungarian_match, matched votes / n."""
    from scipy.optimize import linear_sum_assignment
    x, device = _features_on_device(fvecs, device, "compute_cluster_accuracy")
    y = torch.as_tensor(targets).to(device=device, dtype=torch.int32).contiguous()
    n = x.shape[0]
    if y.shape != (n,):
        raise ValueError(f"expected fvecs [n,d] and targets [n], got {tuple(x.shape)} and {tuple(y.shape)}")
    if num_classes is None:
        num_classes = int(y.max().item()) + 1
    run = kmeans(x, int(num_classes), niter=niter, nredo=nredo, seed=seed, device=device)
    votes = ops.cluster_votes(run["labels"], y, int(num_classes), int(num_classes)).cpu().numpy()
    rows, cols = linear_sum_assignment(n - votes)
    return float(votes[rows, cols].sum()) / float(n)


def knn_classify(train_fvecs, train_labels, test_fvecs, test_labels, k=20, temperature=0.07, num_classes=None, normalize=True, device=None):
    """The weighted k-nearest-neighbour classifier of InstDisc / MoCo / DINO's eval_knn: every test feature searches the TRAIN features (ops.knn_search, exact
    inner product), its k best neighbours vote for their class with weight exp(similarity / temperature) (ops.knn_vote).  numpy arrays or device tensors;
    rows are L2-normalised first (ssv_l2norm_fwd) unless ``normalize`` is False; k is clipped to the number of train rows (tiny synthetic sets);
    ``num_classes`` defaults to train_labels.max() + 1.  Returns {"top1", "top5", "pred"}: accuracies as floats (top5 None with fewer than 5 classes) and
    pred [m, min(5, num_classes)] int32 on the device, best class first - bit for bit what the two ops calls give when composed by hand."""
    bank, device = _features_on_device(train_fvecs, device, "knn_classify")
    queries, _ = _features_on_device(test_fvecs, device, "knn_classify")
    ytr = torch.as_tensor(train_labels).to(device=device, dtype=torch.int32).contiguous()
    yte = torch.as_tensor(test_labels).to(device=device, dtype=torch.int32).contiguous()
    (n, d), m = bank.shape, queries.shape[0]
    if queries.shape[1] != d or ytr.shape != (n,) or yte.shape != (m,):
        raise ValueError(f"knn_classify: expected train [n,d] / [n] and test [m,d] / [m], got {tuple(bank.shape)} / {tuple(ytr.shape)} and {tuple(queries.shape)} / {tuple(yte.shape)}")
    if num_classes is None:
        num_classes = int(ytr.max().item()) + 1
    num_classes, k = int(num_classes), max(1, min(int(k), n))
    if normalize:
        bank, queries = ops.l2norm_fwd(bank)[0], ops.l2norm_fwd(queries)[0]
    sim, idx = ops.knn_search(queries, bank, k)
    topn = min(5, num_classes)
    pred = ops.knn_vote(sim, idx, ytr, num_classes, temperature, topn=topn)
    hit = pred == yte[:, None]
    top1 = float(hit[:, 0].sum().item()) / float(m)
    top5 = float(hit.any(1).sum().item()) / float(m) if num_classes >= 5 else None
    return {"top1": top1, "top5": top5, "pred": pred}


def probe_batches(n, batch_size, epoch, shuffle, seed=420):
    """Sample order of one probe epoch: a seeded permutation per epoch (the reference shuffles with DataLoader(shuffle=True))."""
    if not shuffle:
        order = torch.arange(n)
    else:
        order = torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch))
    return [order[s:s + batch_size] for s in range(0, n, batch_size)]


def linear_evaluation(config, train_data, test_data, num_classes, device):
    """Linear probe on frozen features, on the GPU: nn.Linear -> NLLLoss(log_softmax) trained with SGD(momentum 0.9, weight decay
    1e-6) and a per-epoch cosine schedule, mini-batches of config["batch_size"]; returns the mean per-batch test accuracy of the
    last epoch.  That is the INTENT of utils/eval_utils.py:37-76 - the reference's own function cannot run (its loaders are tuples,
    it averages a bool tensor, and `input_dim` in the shipped configs does not match the feature width), so the width is taken
    from the features.  Logits and the weight gradient run on the MFMA GEMM kernels (classes padded to a multiple of 4)."""
    import math
    from .. import _lib
    if not torch.cuda.is_available():
        raise RuntimeError("linear_evaluation runs on the GPU (libssv_hip); no HIP device is visible and there is no CPU fallback")
    device = device if isinstance(device, torch.device) and device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    to_dev = lambda a, dt: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=device, dtype=dt).contiguous()
    xtr, ytr = to_dev(train_data["fvecs"], torch.float32), to_dev(train_data["labels"], torch.int32)
    xte, yte = to_dev(test_data["fvecs"], torch.float32), to_dev(test_data["labels"], torch.int32)
    for name, y in (("train", ytr), ("test", yte)):
        lo, hi = int(y.min().item()), int(y.max().item())
        if lo < 0 or hi >= num_classes:
            raise ValueError(f"linear_evaluation: {name} labels span [{lo}, {hi}] but num_classes = {num_classes}")
    d = xtr.shape[1]
    if d % 4:
        pad = 4 - d % 4
        xtr, xte = torch.nn.functional.pad(xtr, (0, pad)), torch.nn.functional.pad(xte, (0, pad))
        d += pad
    cpad = (num_classes + 3) // 4 * 4
    head = torch.nn.Linear(train_data["fvecs"].shape[1], num_classes)           # the reference's init draw (CPU RNG)
    flat = torch.zeros(cpad * d + cpad, device=device)                          # [W (cpad x d) | b (cpad)] in one buffer: one optimiser launch
    w, b = flat[:cpad * d].view(cpad, d), flat[cpad * d:]
    w[:num_classes, :head.in_features].copy_(head.weight.detach())
    b[:num_classes].copy_(head.bias.detach())
    grad, buf = torch.zeros_like(flat), torch.zeros_like(flat)
    gw, gb = grad[:cpad * d].view(cpad, d), grad[cpad * d:]
    stats = torch.zeros(2, device=device)
    lr0, epochs, bs = float(config["lr"]), int(config["epochs"]), int(config["batch_size"])
    mom, wd = float(config.get("momentum", 0.9)), float(config.get("weight_decay", 1e-06))
    lib = _lib.load()

    def run(x, y, train, lr, first):
        n = x.shape[0]
        logits = ops.conv2d_fwd(x.view(n, 1, 1, d), w, bias=b).view(n, cpad)
        dlog = torch.empty_like(logits) if train else None
        ws = _lib.workspace.get(lib.ssv_softmax_ce_workspace_bytes(n), device)
        _lib.call("ssv_softmax_ce_fwd_bwd", n, num_classes, cpad, _lib.ptr(logits), _lib.ptr(y), _lib.ptr(stats), _lib.ptr(dlog), _lib.ptr(ws), ws.numel(), _lib.stream())
        if train:
            ops.conv2d_wgrad(x.view(n, 1, 1, d), dlog.view(n, 1, 1, cpad), w, gw, accumulate=False)
            ops.colsum(dlog, gb, accumulate=False)
            _lib.call("ssv_sgd", flat.numel(), _lib.ptr(flat), _lib.ptr(grad), _lib.ptr(buf), lr, wd, mom, 0, int(first), _lib.stream())
            ops.invalidate_weight_caches()         # w changed under its cached bf16 planes (every in-place update of a GEMM operand says so)
        return stats

    acc, step = 0.0, 0
    for epoch in range(1, epochs + 1):
        lr = 0.5 * lr0 * (1.0 + math.cos(math.pi * (epoch - 1) / epochs))      # CosineAnnealingLR(T_max=epochs), stepped once per epoch
        for idx in probe_batches(xtr.shape[0], bs, epoch, True):
            idx = idx.to(device)
            run(xtr[idx], ytr[idx], True, lr, step == 0)
            step += 1
        if epoch == epochs:
            accs = [float(run(xte[idx.to(device)], yte[idx.to(device)], False, 0.0, False)[1]) for idx in probe_batches(xte.shape[0], bs, epoch, False)]
            acc = float(np.mean(accs))
    print("\nCompleted linear evaluation. Average validation accuracy is {:.2f}%".format(100 * acc))
    return acc
