"""The oracle of the DenseCL tests (tests/test_densecl_cpu.py, tests/test_gpu_dense_nce.py, tests/test_gpu_densecl.py and the launch-form files
tests/test_gpu_dense_nce_forms.py, tests/test_gpu_dense_match_forms.py): the dense matching, the queue InfoNCE and the
trainer's combined loss in plain torch under autograd (float64, or the same lines in float32), the case tables the kernel tests run and a restatement of the
kernel's launch plan.  Nothing here touches the GPU or the library.

dense_match (include/ssv_hip.h: ssv_dense_match): per image, j* = argmax_j f1_i . f2_j / max(|f2_j|, eps), lowest j among equal scores; sim = the cosine.
queue_nce (ssv_queue_nce): s_i+ = q_i . keys[pos_i] * inv_temp, s_ij = q_i . bank_j * inv_temp (j < K), lse_i = log(exp(s_i+) + sum_j exp(s_ij)),
    loss = mean_i (lse_i - s_i+), dq = d loss / dq."""
import torch

FUSED_MAX_D = 128                    # SSV_QUEUE_NCE_FUSED_MAX_D
FLOOR = 2 * 2.0 ** -24               # the accuracy rule of tests/test_gpu_dense_nce.py: e(got) <= FACTOR * e(ref32) + FLOOR
FACTOR = 8.0                         # measured there on an MI355X (profiles/dense_nce_kernels_report.json: 4.77 at worst), rounded up to the next power of two
SLICE, MAX_SLICES, TARGET_WGS = 256, 32, 256          # SSV_QUEUE_NCE_SLICE, _MAX_SLICES, _TARGET_WGS
CHUNK_ROWS, CHUNK_ELEMS = 1024, 1 << 25               # the unfused route's query chunk (csrc/densecl.hip)
MAX_M, MATCH_MAX_S = 131072, 256                      # SSV_QUEUE_NCE_MAX_M, SSV_DENSE_MATCH_MAX_S
MATCH_MAX_C = 8192                                    # SSV_DENSE_MATCH_MAX_C
TIE = 8 * 2.0 ** -24                 # a chosen cell whose fp64 cosine is this close to the best one is excused (at most 1 % of a case's cells)


def next_pow2(x):
    p = 1.0
    while p < x:
        p *= 2.0
    return p


# ---- the oracles ------------------------------------------------------------------------------------------------------------------------------------------------
def dense_match(f1, f2, eps=1e-12, dtype=torch.float64):
    """{"j" [b, s] (cell of view 2), "idx" [b, s] = n * s + j, "sim" [b, s], "cos" [b, s, s] (every pair's cosine), "score" [b, s, s]} in ``dtype`` on the CPU"""
    a, c = f1.detach().cpu().to(dtype), f2.detach().cpu().to(dtype)
    b, s = a.shape[0], a.shape[1]
    a, c = a.reshape(b, s, -1), c.reshape(b, s, -1)
    dot = torch.bmm(a, c.transpose(1, 2))
    n1, n2 = a.norm(dim=2).clamp_min(eps), c.norm(dim=2).clamp_min(eps)
    score = dot / n2[:, None, :]
    j = score.argmax(dim=2)                                        # torch returns the first of equal maxima
    best = score.max(dim=2, keepdim=True).values
    j = (score == best).float().argmax(dim=2)                      # ... stated explicitly: the lowest j among equal scores
    cos = dot / (n1[:, :, None] * n2[:, None, :])
    return {"j": j, "idx": j + s * torch.arange(b)[:, None], "sim": cos.gather(2, j[:, :, None])[:, :, 0], "cos": cos, "score": score}


def queue_nce(q, keys, pos, bank, K, inv_temp, dtype=torch.float64, normalize=False):
    """{"loss" 0-d, "lse" [m], "dq" [m, d], "pos" (mean probability of the positive), "smax" (largest |score|)} in ``dtype`` on the CPU.  ``normalize``: the rows of
    q and of keys are divided by max(|.|, 1e-12) first and dq is the gradient with respect to the raw rows of q (utils.losses.DenseNceLoss)."""
    raw = q.detach().cpu().to(dtype).requires_grad_(True)
    kk = keys.detach().cpu().to(dtype)
    if normalize:
        qd, kk = raw / raw.norm(dim=1, keepdim=True).clamp_min(1e-12), kk / kk.norm(dim=1, keepdim=True).clamp_min(1e-12)
    else:
        qd = raw
    bk = bank.detach().cpu().to(dtype)[:int(K)]
    kp = kk[pos.detach().cpu().long()]
    sp = (qd * kp).sum(dim=1) * inv_temp
    sc = torch.cat([sp[:, None], (qd @ bk.T) * inv_temp], dim=1)
    lse = torch.logsumexp(sc, dim=1)
    loss = (lse - sp).mean()
    loss.backward()
    return {"loss": loss.detach(), "lse": lse.detach(), "dq": raw.grad.detach(), "pos": float(torch.exp(sp - lse).detach().mean()), "smax": float(sc.detach().abs().max())}


def moco_loss(q, k, bank, K, temperature, dtype=torch.float64):
    """MoCo's InfoNCE on raw embeddings (both L2-normalised here): {"loss", "dq"}"""
    raw = q.detach().cpu().to(dtype).requires_grad_(True)
    kk = k.detach().cpu().to(dtype)
    qd, kd = raw / raw.norm(dim=1, keepdim=True).clamp_min(1e-12), kk / kk.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sc = torch.cat([(qd * kd).sum(dim=1, keepdim=True), qd @ bank.detach().cpu().to(dtype)[:int(K)].T], dim=1) / temperature
    loss = (torch.logsumexp(sc, dim=1) - sc[:, 0]).mean()
    loss.backward()
    return {"loss": loss.detach(), "dq": raw.grad.detach()}


def densecl_loss(q, k, bank, K, grid_q, grid_k, pos, dense_bank, dense_K, temperature, lam, dtype=torch.float64):
    """The trainer's loss on raw embeddings: (1 - lam) * MoCo(q, k, queue) + lam * dense(grid_q, grid_k[pos], dense queue); {"loss", "global", "dense"}"""
    g = moco_loss(q, k, bank, K, temperature, dtype)["loss"]
    d = queue_nce(grid_q, grid_k, pos, dense_bank, dense_K, 1.0 / temperature, dtype, normalize=True)["loss"]
    return {"loss": (1.0 - lam) * g + lam * d, "global": g, "dense": d}


def errs(got, ref):
    """(|got - ref|_2 / |ref|_2, max|got - ref| / max|ref|) in float64; a zero reference gives 0 for an exact match and inf otherwise"""
    g, r = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    dn, dm, rn, rm = float((g - r).norm()), float((g - r).abs().max()), float(r.norm()), float(r.abs().max())
    if rn == 0.0:
        return (0.0, 0.0) if dn == 0.0 else (float("inf"), float("inf"))
    return dn / rn, dm / rm


# ---- the plan of ssv_queue_nce restated (csrc/densecl.hip: make_plan and the dispatch) ----------------------------------------------------------------------------
def plan(m, K, d, arith):
    """{"fused", "bytes"} and, fused, DT and KT (the template arguments), T (query tiles), blocks, slices and rows (of one slice); unfused, cr (query rows of a
    chunk), chunks and kp (rows of the padded copy of the queue)"""
    cdiv, up = lambda a, b: -(-a // b), lambda v: (v + 255) // 256 * 256
    rl = up(m * 8)
    if arith == "bf16x3" and d % 32 == 0 and d <= FUSED_MAX_D:
        t, dt = cdiv(m, 32), d // 32
        kt = 1 if t == 1 or dt >= 3 else 2
        blocks, units = cdiv(t, kt), cdiv(K, SLICE)
        want = min(MAX_SLICES, cdiv(TARGET_WGS, blocks), units)
        rows = SLICE * cdiv(units, want)
        nsl = cdiv(K, rows)
        return {"fused": True, "DT": dt, "KT": kt, "T": t, "blocks": blocks, "slices": nsl, "rows": rows,
                "bytes": rl + 2 * up(4 * nsl * 32 * t * 4) + up(4 * nsl * 32 * t * d * 4) + 3 * (d // 16) * t * 1024}
    kp = (K + 15) // 16 * 16
    cr = max(1, min(CHUNK_ELEMS // kp, CHUNK_ROWS, m))
    return {"fused": False, "cr": cr, "chunks": cdiv(m, cr), "kp": kp, "bytes": rl + up(cr * kp * 4) + up(kp * d * 4)}


# ---- the case tables --------------------------------------------------------------------------------------------------------------------------------------------
MS = (1, 33, 70)                                      # one query, one tile and a row, two tiles and a ragged third
DS = (32, 64, 96, 128, 4, 36, 160)                    # the fused widths; 4, 36 and 160 take the unfused route in either arithmetic (160 is a multiple of 32)
KS = (1, 31, 33, 513, 640)                            # one row, below a tile, a tile and a row, two slices and a row, a multiple of 16 with a ragged last slice
VARIANTS = ("plain", "same", "late", "dup", "zero")
# just past the m-thresholds of the plan at K = 640 (three slices up to 127 blocks, two up to 255, then one; blocks = tiles at d >= 96, tiles / 2 below),
# and more than one chunk of the unfused route
BIG = [(4129, 128, 640, "plain"), (8225, 128, 640, "plain"), (8225, 64, 640, "plain"), (16417, 64, 640, "plain"), (8225, 36, 640, "plain"), (1030, 160, 513, "plain"),
       (1030, 4, 33, "plain")]
ROUTES_AGREE = [(70, 128, 640, "plain"), (33, 32, 513, "plain"), (70, 96, 640, "late"), (70, 128, 640, "dup")]


def cases():
    """(m, d, K, variant): every m x d x K plain, the planted variants at the shapes where they mean something, and the large-m forms"""
    out = [(m, d, k, "plain") for k in KS for d in DS for m in MS]
    for d in (128, 96, 36):
        for v in VARIANTS[1:]:
            out.append((70, d, 640, v))
    out.append((33, 64, 1, "zero"))
    return out + BIG


def case_id(case):
    m, d, k, variant = case
    return f"m{m}-d{d}-k{k}-{variant}"


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def make_case(case, seed=0):
    """(q [m, d], keys [mk, d], pos int32 [m], bank [K, d], K, inv_temp): fp32 unit rows (|q . k| <= 1) and inv_temp = 5 (a temperature of 0.2), so |s| <= 5
    (the variant `climb`: CLIMB_INV_TEMP); mk = m + 3; pos at the first key, at the last, otherwise drawn.  The positive leans on its query (cosine about 0.3),
    as a matched cell does."""
    m, d, K, variant = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + 13 * d + K)
    mk = m + 3
    q = _unit(torch.randn(m, d, generator=g, dtype=torch.float64))
    keys = _unit(torch.randn(mk, d, generator=g, dtype=torch.float64))
    bank = _unit(torch.randn(K, d, generator=g, dtype=torch.float64))
    drawn = torch.randint(0, mk, (m,), generator=g).tolist()
    pos = torch.tensor([(0, mk - 1, drawn[i])[i % 3] for i in range(m)], dtype=torch.int32)
    if variant == "same":                              # every query has the same positive
        pos[:] = mk // 2
    else:
        for i in range(2, m, 3):
            keys[drawn[i]] = _unit((keys[drawn[i]] + 0.3 * q[i])[None])[0]
    if variant == "dup":                               # rows 255 | 256 lie in two slices (and two workgroups): the same row twice
        bank[256] = bank[255]
    if variant == "late":                              # every query leans towards one direction, which is the LAST bank row: the running maximum is replaced in the last tile
        lean = _unit(torch.randn(1, d, generator=g, dtype=torch.float64))
        q = _unit(q + 1.5 * lean)
        bank[K - 1] = lean[0]
    if variant == "zero":                              # the fresh queue
        bank.zero_()
    if variant == "dupL":                              # as dup, at the boundary of the bf16x3 plan's LONG slices (FORM_CASES: rows FORM_DUP_ROW - 1 | FORM_DUP_ROW)
        bank[FORM_DUP_ROW] = bank[FORM_DUP_ROW - 1]
    if variant == "climb":                             # the queries lean on one direction and the bank rows are sorted ascending by their product with it: the
        lean = _unit(torch.randn(1, d, generator=g, dtype=torch.float64))      # running maximum is replaced tile after tile, at a temperature of 0.07
        q = _unit(q + 1.5 * lean)
        bank = bank[torch.argsort(bank @ lean[0])]
    return q.float(), keys.float(), pos, bank.float(), K, (CLIMB_INV_TEMP if variant == "climb" else 5.0)


# ---- the launch forms (tests/test_gpu_dense_nce_forms.py) ----------------------------------------------------------------------------------------------------
LONG = 8200                                           # past SLICE * MAX_SLICES rows: slices of 2 * SLICE rows, 17 of them, the last of 8 rows
FORM_DUP_ROW = 2 * SLICE                              # the first row of the second slice of that plan
CLIMB_INV_TEMP = 1.0 / 0.07
CLAMP = 32800                                         # a multiple of 16 above 2^25 / 1024: the chunk of the unfused route is 2^25 // 32800 = 1023 rows
FORM_CASES = [(33, 32, LONG, "plain"), (33, 128, LONG, "late"), (1, 64, LONG, "plain"), (97, 64, LONG, "dupL"), (33, 36, LONG, "plain"),
              (70, 64, 255, "plain"), (70, 64, 256, "plain"), (70, 64, 257, "plain"),
              (70, 96, 65, "plain"), (70, 32, 129, "plain"), (70, 128, 193, "plain"),
              (1030, 4, CLAMP, "plain"), (1030, 36, CLAMP, "plain"),
              (70, 96, 640, "climb"), (70, 64, LONG, "climb"), (33, 128, LONG, "climb"), (70, 36, 640, "climb"),
              (MAX_M, 32, 33, "plain")]
FORM_ROUTES_AGREE = [(33, 128, LONG, "late"), (70, 64, LONG, "climb")]


def climbing_tiles(q, bank):
    """(the mean over the queries of the number of 32-row tiles whose largest score is above that of every tile before them, the number of tiles)"""
    sc = q.double() @ bank.double().T
    tiles = -(-sc.shape[1] // 32)
    top = torch.stack([sc[:, 32 * t:32 * t + 32].max(dim=1).values for t in range(tiles)], dim=1)
    raised = top[:, 1:] > torch.cummax(top, dim=1).values[:, :-1]
    return float(raised.sum(dim=1).double().mean()), tiles


MATCH_CASES = [(3, 1, 8, "plain"), (5, 16, 64, "plain"), (4, 49, 512, "plain"), (3, 50, 36, "plain"), (2, 256, 128, "plain"), (1, 256, 2048, "plain"),
               (5, 16, 64, "planted"), (2, 256, 128, "planted")]
MATCH_SEEDS = (0, 1, 2)


def match_id(case):
    b, s, c, variant = case
    return f"b{b}-s{s}-c{c}-{variant}"


# the launch forms of dm_match_k (tests/test_gpu_dense_match_forms.py): (b, s, c, variant)
FORM_MATCH_CASES = [(2, 32, 64, "plain"), (3, 33, 64, "plain"), (2, 64, 36, "plain"), (7, 65, 64, "plain"), (2, 96, 64, "plain"), (2, 97, 64, "plain"),
                    (2, 128, 128, "plain"), (2, 129, 128, "plain"), (1, 160, 64, "plain"), (1, 255, 64, "plain"),
                    (2, 256, 64, "perm"), (2, 129, 128, "perm"), (2, 33, 36, "perm"),
                    (2, 256, 64, "ties"),
                    (2, 50, 64, "eps"), (1, 256, 128, "eps"),
                    (2, 50, 64, "nan"),
                    (3, 16, 4, "signed"), (3, 16, 12, "signed"), (2, 50, 24, "signed"), (2, 129, 8, "signed"), (1, 33, MATCH_MAX_C, "plain")]
MATCH_EPS = 0.5                                       # the eps of the variant `eps`; every other case calls with 1e-12
TIES = {37: 5, 133: 5, 165: 5, 130: 100}              # variant `ties`, image 0: cell of f2 -> the cell it is a copy of
TIES_F1 = {0: 5, 40: 5, 1: 100, 255: 100}             # ... and cell of f1 -> the cell of f2 it is a copy of
NAN_CELL = (1, 7, 3)                                  # variant `nan`: (image, cell, channel) of f1


def match_eps(case):
    return MATCH_EPS if case[3] == "eps" else 1e-12


def make_match_case(case, seed=0):
    """(f1, f2) [b, s, c] fp32: ReLU of standard normal features, as a backbone's are.  planted: in image 0 cell 7 of f2 is a copy of cell 3 (an exact tie, which
    must resolve to 3) and cell 0 of f1 is that cell too; in the last image row 1 of f1 is zero (it picks j = 0) and row 2 of f2 is zero (it is never chosen over a positive score).
    The variants of FORM_MATCH_CASES -
    signed: no ReLU (at c = 4 the ReLU leaves all-zero rows, which tie at 0);
    perm:   f1[n] = f2[n][p[n]] for drawn permutations p (match_perm): by Cauchy-Schwarz the arg-max of cell i is p[n][i] and its cosine 1;
    ties:   in image 0 the cells TIES of f2 are copies of lower cells and the cells TIES_F1 of f1 are copies of those originals;
    eps:    every second cell of f2 is scaled by 0.01 and the call takes eps = MATCH_EPS, which is returned as a third element: (f1, f2, eps);
    nan:    one channel of one cell of f1 (NAN_CELL) is NaN."""
    b, s, c, variant = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * b + 13 * s + c)
    f1 = torch.randn(b, s, c, generator=g)
    f2 = torch.randn(b, s, c, generator=g)
    if variant != "signed":
        f1, f2 = torch.relu(f1), torch.relu(f2)
    if variant == "planted":
        f2[0, 7] = f2[0, 3]
        f1[0, 0] = f2[0, 3]                            # cell 0 of image 0 certainly matches the duplicated cell
        f1[b - 1, 1] = 0.0
        f2[b - 1, 2] = 0.0
    if variant == "perm":
        p = torch.stack([torch.randperm(s, generator=g) for _ in range(b)])
        f1 = torch.gather(f2, 1, p[:, :, None].expand(b, s, c))
    if variant == "ties":
        for copy, orig in TIES.items():
            f2[0, copy] = f2[0, orig]
        for cell, orig in TIES_F1.items():
            f1[0, cell] = f2[0, orig]
    if variant == "nan":
        f1[NAN_CELL] = float("nan")
    if variant == "eps":
        f2[:, ::2] *= 0.01
        return f1.contiguous(), f2.contiguous(), MATCH_EPS
    return f1.contiguous(), f2.contiguous()


def match_perm(case, seed=0):
    """the permutations [b, s] the variant `perm` drew: make_match_case's generator after its two draws"""
    b, s, c, variant = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * b + 13 * s + c)
    torch.randn(b, s, c, generator=g), torch.randn(b, s, c, generator=g)
    return torch.stack([torch.randperm(s, generator=g) for _ in range(b)])


def match_gap(case, ref):
    """The smallest fp64 gap between the best and the second-best cosine over the cells that have one: a planted copy counts as its original, an all-zero
    f1 row has no best and neither has a cell of f1 that holds a NaN"""
    b, s, c, variant = case
    cos = ref["cos"].clone()
    if s < 2:
        return float("inf")
    if variant == "planted":
        cos[0, :, 7] = -1.0
    if variant == "ties":
        cos[0, :, list(TIES)] = -1.0
    if variant == "nan":
        cos[NAN_CELL[0], NAN_CELL[1]] = 0.0
    top = cos.topk(2, dim=2).values
    gap = top[:, :, 0] - top[:, :, 1]
    if variant == "planted":
        gap[b - 1, 1] = float("inf")
    if variant == "nan":
        gap[NAN_CELL[0], NAN_CELL[1]] = float("inf")
    return float(gap.min())
