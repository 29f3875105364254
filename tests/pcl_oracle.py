"""The oracle of the PCL tests (tests/test_pcl_cpu.py, tests/test_gpu_proto_nce.py, tests/test_gpu_pcl.py): ProtoNCE in plain torch under autograd (float64, or the
same lines in float32), PCL's concentration in numpy float64, and the case table the kernel tests run.  Nothing here touches the GPU or the library.

ProtoNCE (include/ssv_hip.h: ssv_proto_nce): prototypes [ktot, d] cut into segments by seg_end, s_ij = (q_i . c_j) * inv_phi_j, labels [segs, m] inside each segment;
    lse[s, i] = logsumexp_{j in segment s} s_ij,   loss = 1 / segs * sum_s mean_i (lse[s, i] - s_iy),   dq = d loss / dq."""
import math

import numpy as np
import torch

FUSED_MAX_D = 128                    # SSV_PROTO_NCE_FUSED_MAX_D
FLOOR = 2 * 2.0 ** -24               # the accuracy rule of tests/test_gpu_proto_nce.py: e(got) <= FACTOR * e(ref32) + FLOOR
FACTOR = 4.0                         # measured there on an MI355X (worst ratio 2.85), rounded up to the next power of two
SLICE = 256                          # SSV_PROTO_NCE_SLICE: rows of one slice of a segment on the fused route (a wave takes a quarter, 32 rows at a time)


def proto_nce(q, protos, inv_phi, labels, seg_end, dtype=torch.float64, normalize=False):
    """{"loss" 0-d, "lse" [segs, m], "dq" [m, d], "pos" (mean probability of the positive), "smax" (largest |score|)} in ``dtype`` on the CPU.  ``normalize``: the
    rows of q are divided by max(|q|, 1e-12) first and dq is the gradient with respect to the raw rows (utils.losses.ProtoNceLoss)."""
    raw = q.detach().cpu().to(dtype).requires_grad_(True)
    qd = raw / raw.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else raw
    c, ip = protos.detach().cpu().to(dtype), inv_phi.detach().cpu().to(dtype)
    lab = labels.detach().cpu().long()
    m = qd.shape[0]
    total, lses, pos, smax, b = 0.0, [], [], 0.0, 0
    for s, e in enumerate(int(v) for v in seg_end):
        sc = (qd @ c[b:e].T) * ip[b:e]
        lse = torch.logsumexp(sc, dim=1)
        sy = sc[torch.arange(m), lab[s]]
        total = total + (lse - sy).mean()
        lses.append(lse.detach())
        pos.append(torch.exp(sy - lse).detach())
        smax = max(smax, float(sc.detach().abs().max()))
        b = e
    loss = total / len(lses)
    loss.backward()
    return {"loss": loss.detach(), "lse": torch.stack(lses), "dq": raw.grad.detach(), "pos": float(torch.stack(pos).mean()), "smax": smax}


def errs(got, ref):
    """(|got - ref|_2 / |ref|_2, max|got - ref| / max|ref|) in float64; a zero reference gives 0 for an exact match and inf otherwise"""
    g, r = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    dn, dm, rn, rm = float((g - r).norm()), float((g - r).abs().max()), float(r.norm()), float(r.abs().max())
    if rn == 0.0:
        return (0.0, 0.0) if dn == 0.0 else (float("inf"), float("inf"))
    return dn / rn, dm / rm


# ---- the case table -------------------------------------------------------------------------------------------------------------------------------------------
MS = (1, 33, 70)                                      # one query, one tile and a row, two tiles and a ragged third
DS = (32, 64, 128, 4, 36)                             # the fused widths up to its maximum; 4 and 36 take the unfused route in either arithmetic
SEGSETS = ((31,), (33,), (513,), (7, 33, 600), (1, 33))        # below a tile, a tile and a row, two slices and a row, three segments with a slice boundary in the last, a one-prototype segment beside another
VARIANTS = ("plain", "dup", "late")                   # dup: a prototype duplicated across the slice boundary at row 256; late: the largest score sits in the last slice


def cases():
    """(m, d, sizes, variant): every m x d x segment set plain, and the two planted variants at the shapes where they mean something"""
    out = [(m, d, sizes, "plain") for sizes in SEGSETS for d in DS for m in MS]
    for d in (128, 36):
        out.append((70, d, (513,), "dup"))
        out.append((70, d, (7, 33, 600), "late"))
    return out


# ---- the launch forms (tests/test_gpu_proto_nce_forms.py): the smallest shapes that reach each form of csrc/protonce.hip the table above leaves out
EIGHT = (1, 2, 31, 32, 33, 255, 256, 257)             # SSV_PROTO_NCE_MAX_SEGS segments: below, at and above a tile; below, at and above a slice
LONG = 8200                                           # above SLICE * MAX_SLICES rows a slice doubles: 17 slices of 512, the last holding 8 rows
FORM_CASES = [(1, 96, (33,), "plain"), (33, 96, (513,), "plain"), (70, 96, (7, 33, 600), "plain"), (70, 96, (513,), "dup"), (70, 96, (7, 33, 600), "late"),
              (70, 160, (7, 33, 600), "plain"),
              (70, 32, EIGHT, "plain"), (70, 36, EIGHT, "plain"),
              (70, 64, (255,), "plain"), (70, 64, (256,), "plain"), (70, 64, (257,), "plain"),
              (33, 32, (LONG,), "plain"), (33, 128, (LONG,), "late"),
              (1030, 4, (7, 33), "plain"), (1030, 36, (7, 33), "plain"), (1030, 32, (7, 33), "plain")]
FORM_ROUTES_AGREE = [(70, 96, (7, 33, 600), "plain"), (33, 128, (LONG,), "late")]
FORM_SEEDS = (0, 1, 2)                                # the seeds tests/test_pcl_cpu.py checks the reference-side conditions at; the GPU runs seed 0
MAX_SLICES, MAX_SEGS, CHUNK_ROWS = 32, 8, 1024        # SSV_PROTO_NCE_MAX_SLICES, SSV_PROTO_NCE_MAX_SEGS; the unfused route's query chunk


def plan(m, d, sizes, arith):
    """The launch plan of ssv_proto_nce restated (csrc/protonce.hip: make_plan, read_segments and the dispatch): {"fused", "bytes"} and, fused, DT and KT (the
    template arguments), T (query tiles), blocks, rows / first (rows of one slice and first slice of every segment; first[-1] = all slices); unfused, cr (query rows
    of a chunk), chunks and kp (rows of the padded copy of every segment)."""
    cdiv, up = lambda a, b: -(-a // b), lambda v: (v + 255) // 256 * 256
    segs, ktot = len(sizes), sum(sizes)
    common = up(segs * cdiv(m, 32) * 32 * 4) + up(segs * m * 4)
    if arith == "bf16x3" and d % 32 == 0 and d <= FUSED_MAX_D:
        t, dt = cdiv(m, 32), d // 32
        kt = 1 if t == 1 or dt >= 3 else 2
        rows = [SLICE * cdiv(cdiv(k, SLICE), MAX_SLICES) for k in sizes]
        first = [0]
        for k, r in zip(sizes, rows):
            first.append(first[-1] + cdiv(k, r))
        worst = min(cdiv(ktot, SLICE) + segs, MAX_SLICES * segs)
        return {"fused": True, "DT": dt, "KT": kt, "T": t, "blocks": cdiv(t, kt), "rows": rows, "first": first,
                "bytes": common + 2 * up(4 * worst * 32 * t * 4) + up(4 * worst * 32 * t * d * 4) + 3 * (d // 16) * t * 1024}
    longest = (ktot - (segs - 1) + 15) // 16 * 16
    cr = max(1, min((1 << 25) // longest, CHUNK_ROWS, m))
    return {"fused": False, "cr": cr, "chunks": cdiv(m, cr), "kp": [(k + 15) // 16 * 16 for k in sizes], "bytes": common + up(cr * longest * 4) + up(longest * d * 4)}


def case_id(case):
    m, d, sizes, variant = case
    return f"m{m}-d{d}-k{'_'.join(map(str, sizes))}-{variant}"


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def make_case(case, seed=0):
    """(q [m, d], protos [ktot, d], inv_phi [ktot], labels int32 [segs, m], seg_end): fp32 unit rows (|q . c| <= 1, so |s| <= 20), inv_phi log-uniform in [2, 20];
    labels at the first prototype of a segment, at the last, inside the last partial tile of 32, otherwise drawn."""
    m, d, sizes, variant = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + 13 * d + sum(sizes))
    ktot = sum(sizes)
    q = _unit(torch.randn(m, d, generator=g, dtype=torch.float64))
    protos = _unit(torch.randn(ktot, d, generator=g, dtype=torch.float64))
    inv_phi = torch.exp(torch.rand(ktot, generator=g, dtype=torch.float64) * math.log(10.0) + math.log(2.0))
    seg_end = tuple(int(v) for v in np.cumsum(sizes))
    labels = torch.empty(len(sizes), m, dtype=torch.int32)
    for s, k in enumerate(sizes):
        drawn = torch.randint(0, k, (m,), generator=g)
        for i in range(m):
            labels[s, i] = (0, k - 1, min(k - 1, (k - 1) // 32 * 32 + i % 5), int(drawn[i]))[i % 4]
    if variant == "dup":                               # rows 255 | 256 lie in two slices (and two workgroups): the same prototype with the same concentration
        protos[256], inv_phi[256] = protos[255], inv_phi[255]
    if variant == "late":                              # every query leans towards one direction, which is the LAST prototype: the running maximum is replaced in the last slice
        lean = _unit(torch.randn(1, d, generator=g, dtype=torch.float64))
        q = _unit(q + 1.5 * lean)
        protos[ktot - 1], inv_phi[ktot - 1] = lean[0], 20.0
    return q.float(), protos.float(), inv_phi.float(), labels, seg_end


# ---- PCL's concentration ----------------------------------------------------------------------------------------------------------------------------------------
def cluster_concentration(dist, labels, counts, alpha=10.0, temperature=0.2):
    """numpy float64 restatement of eval_utils.cluster_concentration (the authors' run_kmeans): phi [k]"""
    dist, labels, counts = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t) for t in (dist, labels, counts))
    k = counts.shape[0]
    root = np.sqrt(np.maximum(dist.astype(np.float64), 0.0))
    phi = np.zeros(k, dtype=np.float64)
    for j in range(k):
        members = root[labels == j]
        assert members.shape[0] == counts[j]
        if counts[j] > 1:
            phi[j] = members.mean() / math.log(counts[j] + alpha)
    many = counts > 1
    top = phi[many].max() if many.any() else 1.0
    phi[~many] = top
    phi = np.clip(phi, np.percentile(phi, 10), np.percentile(phi, 90))
    return temperature * phi / phi.mean()


def blobs(n=300, d=16, k=12, seed=0):
    """(x [n, d] fp32, centres [k, d] fp32): Gaussian blobs of unequal spread, one centre without a member and one with a single member"""
    g = torch.Generator().manual_seed(seed)
    centres = 4.0 * torch.randn(k, d, generator=g)
    centres[k - 1] = 100.0                                                # nobody is assigned to it
    owner = torch.randint(0, k - 2, (n,), generator=g)
    spread = 0.2 + 0.1 * owner.float()
    x = centres[owner] + spread[:, None] * torch.randn(n, d, generator=g)
    x[0] = centres[k - 2] + 0.01                                          # the only member of cluster k - 2
    return x.contiguous(), centres.contiguous()
