"""Every loss, normalisation and optimizer kernel between the encoder and the parameter update (csrc/loss.hip, siblings.hip, dino.hip, optim.hip, the
soft-max cross-entropy of evalknn.hip, ssv_fill of runtime.hip) against an fp64 evaluation of the same operation on the same fp32 inputs.

Each case of CASES names the entry points it reaches (straight through the C ABI where a kernel has an entry point of its own; through ops.* /
utils.losses.* where the host composes several kernels, so that the composition is under the same bar), the branch labels it targets and a shape.
Cases whose composition contains a GEMM (MoCo, Barlow Twins, the wide NT-Xent route) run once under ops.arithmetic("f32") and once under ("bf16x3").
The inputs are drawn on the CPU from a generator seeded by the case id, so the GPU-free tests below see exactly what the GPU tests upload.  Every run is
held to:

  (a) for every tensor (and the loss scalar) a case produces, with ref64 = plain torch in float64 on the CPU, ref32 = the SAME lines in float32 on the
      CPU, e(x) = ||x - ref64||_2 / ||ref64||_2 and m(x) = max|x - ref64| / max|ref64|:
          e(got) <= FACTOR[family] * e(ref32) + FLOOR[family]     and the same for m.
      e(ref32) comes from the reference, never from the library.  Scalars the C ABI takes as float (temperatures, learning rates, ...) enter both
      references as the fp32 value the kernel receives.  FACTOR / FLOOR: one pair per family, see below;
  (b) a condition on the inputs: ref32 itself is within 1e-3 of ref64 (e and m) and the fp64 loss is finite - otherwise the case measures nothing
      (test_reference_is_well_conditioned, GPU-free);
  (c) the loss scalar under rule (a);
  (d) every output of a direct C-ABI call is a view into a NaN-prefilled buffer with 1024 floats of guard behind it: no output element stays NaN, the
      guard is untouched, every input is bit-identical afterwards (except `neg` of ssv_moco_loss_fwd_bwd and `S` of ssv_ntxent_gram_weights, which the ABI
      documents as overwritten); workspaces are sized by the library's own *_workspace_bytes where it has one and guarded the same way;
  (e) the bitwise identities the code states: device-memory hyper-parameter forms (ssv_sgd_nesterov_dev, ssv_adamw_counted, ssv_adamw_counted_dev,
      ssv_queue_push_counted) == the host-argument forms, accumulate on a zero prior == overwrite, a second identical call == the first, the loss
      modules == the composition spelled out here.

FACTOR and FLOOR.  A kernel may sum in another order and uses expf / logf of the device library, which moves its error against fp64 by a small factor
either way; an algorithmic mistake (a dropped wave, a stride, `< ldk` for `< K`, a lost max subtraction) moves it by orders of magnitude.  FACTOR is the
worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured per family on an MI355X (profiles/loss_kernels_report.json, written by this file
under SSV_LOSS_REPORT=<path>), rounded up to the next power of two and never above 8.  FLOOR covers outputs whose fp32 reference is exact or luckily tiny
(a single rounding, an element-wise product): any fp32 result carries its own final rounding, so a few 2^-24 is the resolution of the comparison itself;
it is at most 16 * 2^-24.

Branch labels (label, entry points, what the case reaches) - test_case_table_covers_every_documented_branch keeps CASES honest:

  moco.config          ssv_moco_loss_fwd_bwd         N 256, K 1000, D 128, T 0.07: the shipped configuration; K > 256 (second trip of the j += 256 loops)
  moco.tiny            ssv_moco_loss_fwd_bwd         N 9, K 50, D 32: one trip of every loop
  moco.ragged_pad      ssv_moco_loss_fwd_bwd         K 4099 in a 4112-row bank whose padding rows hold 1e4: columns >= K masked, neg[:, K:ldk] == 0
  moco.d_trips         ssv_moco_loss_fwd_bwd         D 320 > 256: second trip of the positive dot product and of dq_init
  moco.k65536          ssv_moco_loss_fwd_bwd         K 65536: 256 trips, ldk == K
  moco.unnormalised    ssv_moco_loss_fwd_bwd         normalize 0, T 1.0, inputs x 6: logits of several hundred (max subtraction)
  moco.zero_bank       ssv_moco_loss_fwd_bwd         the step-0 queue: all-zero rows
  relic.config         ssv_relic_kl_fwd_bwd          N 512, D 128
  relic.tiny           ssv_relic_kl_fwd_bwd          N 10, D 32
  relic.n_trips        ssv_relic_kl_fwd_bwd          N 1500 / 4096 > 1024: second trip of the single block's loops
  relic.ragged         ssv_relic_kl_fwd_bwd          N 13 (N % 4 != 0), D 100 (D % 64 != 0), unnormalised
  relic.accumulate     ssv_relic_kl_fwd_bwd          accumulate_loss 1 on a non-zero prior
  relic.whole          RelicLoss                     NT-Xent + invariance term through utils.losses.RelicLoss
  negdot.small         ssv_negdot_pair_fwd_bwd       12 x 64, 7 x 33: one block
  negdot.blocks        ssv_negdot_pair_fwd_bwd       512 x 1024: 512 blocks
  negdot.stride        ssv_negdot_pair_fwd_bwd       512 x 4096 > 2^20 elements: second trip of the grid-stride loop
  mse.small            ssv_mse_pair_fwd_bwd          16 x 128, 7 x 33
  mse.blocks           ssv_mse_pair_fwd_bwd          512 x 128
  mse.stride           ssv_mse_pair_fwd_bwd          512 x 4096: second trip of the grid-stride loop
  barlow.cgrad_min     ssv_barlow_cgrad              D 16, 48: the smallest legal widths
  barlow.cgrad         ssv_barlow_cgrad              D 128, 1000 (D * D not a multiple of 256)
  barlow.cgrad_stride  ssv_barlow_cgrad              D 4096: 16 trips of the grid-stride loop
  barlow.whole         BarlowLoss                    l2norm + BN + three GEMMs + ssv_barlow_cgrad through utils.losses.BarlowLoss
  dino.config          ssv_dino_loss                 bs 64, V 8, K 1024
  dino.k_ragged        ssv_dino_loss                 K 1000 / 257: K % 256 != 0 above 256
  dino.k65536          ssv_dino_loss                 K 65536
  dino.v2              ssv_dino_loss                 V 2
  dino.k64             ssv_dino_loss                 K 64 < one block
  dino.centre          ssv_dino_loss                 a centre of magnitude 5
  dino.weight_acc      ssv_dino_loss                 weight != 1 with accumulate_loss on a non-zero prior
  dino.center_one      ssv_dino_center_update        rows2 = 0 (one teacher block)
  dino.center_two      ssv_dino_center_update        two teacher blocks, K 257 and 65536
  ntxent.online_max    SimclrLoss                    unnormalised inputs, logits of several hundred: the online max subtraction
  ntxent.padded        SimclrLoss                    D 70 -> 96, D 20 -> 32: zero-padded columns
  ntxent.wide          SimclrLoss                    D 512: Gram block from the GEMM, ssv_ntxent_gram_fwd / _weights, dZ as a GEMM
  l2norm.ragged        ssv_l2norm_fwd                D 100 -> ldo 128, rows % 4 != 0
  l2norm.small_d       ssv_l2norm_fwd                D 20 < 64
  l2norm.wide          ssv_l2norm_fwd                D 4096, rows 258
  l2norm.zero_row      ssv_l2norm_fwd                an all-zero row: the eps clamp
  l2norm.copy_padded   ssv_l2norm_fwd                normalize 0 with ldo > D
  wn.config            ssv_weightnorm_fwd            1024 x 512
  wn.ragged            ssv_weightnorm_fwd            1023 x 130, 5 x 63: rows % 4 != 0, cols % 64 != 0
  wn.overwrite         ssv_weightnorm_bwd            accumulate 0 on NaN-prefilled dg / dv
  wn.accumulate        ssv_weightnorm_bwd            accumulate 1 on a seeded prior
  ce.small             ssv_softmax_ce_fwd_bwd        37 x 10 / 256 x 10, ld 12
  ce.c_trips           ssv_softmax_ce_fwd_bwd        C 1000 / 700: several trips of the c += 64 loops
  ce.ragged_rows       ssv_softmax_ce_fwd_bwd        N 129 (N % 4 != 0) with ld == C
  sgdn.tail            ssv_sgd_nesterov              n % 4 != 0 without g2: the scalar tail
  sgdn.tail_g2         ssv_sgd_nesterov              n % 4 != 0 with g2
  sgdn.stride          ssv_sgd_nesterov              n = 2^22 + 3: past the 2048-block cap, with a tail
  sgdn.dev_bitwise     ssv_sgd_nesterov_dev          hyper-parameters in device memory, outside a graph: the same bits
  sgd.plain            ssv_sgd                       nesterov 0
  sgd.nesterov         ssv_sgd                       nesterov 1
  sgd.stride           ssv_sgd                       n = 2^22 + 3
  adamw.g2             ssv_adamw                     second gradient slab
  adamw.clip0          ssv_adamw                     clip 0: no clamp
  adamw.clip3          ssv_adamw                     clip 3
  adamw.counted        ssv_adamw_counted             step count in device memory: the same bits, counter + 1 per call
  adamw.counted_dev    ssv_adamw_counted_dev         learning rate and weight decay in device memory too
  elt.ema              ssv_ema                       n = 5, 1001, 4099, 2^22 + 3
  elt.add              ssv_add                       exact
  elt.scale            ssv_scale                     exact
  elt.fill             ssv_fill                      exact
  queue.counted        ssv_queue_push_counted        pointer in device memory == ssv_queue_push == the sequential loop
  queue.wrap           ssv_queue_push_counted        K 40: pushes of 16, 16, 16 wrap around
  queue.n_gt_k         ssv_queue_push_counted        a push of 90 > K keys

Measured on an MI355X (profiles/loss_kernels_report.json): see FACTOR / FLOOR below and DESIGN.md section 2.
"""
import json
import math
import os
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GUARD = 1024                                                             # floats of NaN behind every output
# one pair per family, set by the rule of the docstring from the MI355X run committed as profiles/loss_kernels_report.json.  Measured worst ratios:
# loss-softmax 4.05 (MoCo, K 65536: dq after the GEMM), loss-elementwise 3.26 (BarlowLoss 1024 x 2048), normalisation 0.19, optimizer 0.61.
FACTOR = {"loss-softmax": 8.0, "loss-elementwise": 4.0, "normalisation": 1.0, "optimizer": 1.0}
# the final rounding of an fp32 result (2^-24 relative), twice where a prior is added: the resolution of the comparison, for every family
FLOOR = {"loss-softmax": 2 * U, "loss-elementwise": 2 * U, "normalisation": 2 * U, "optimizer": 2 * U}
COND = 1e-3                                                              # (b): ref32 further than this from ref64 measures nothing
REPORT = {}                                                              # case id [arith] -> tensor -> figures (SSV_LOSS_REPORT)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-supervised-vision_amd", "csrc")
BIG = 2 ** 22 + 3                                                        # past the 2048-block cap of optim.hip's grid_for, with a tail


def _s(x):
    """a scalar as the C ABI's float argument carries it"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _fmt(v):
    if isinstance(v, bool):
        return "y" if v else "n"
    if isinstance(v, (tuple, list)):
        return "x".join(_fmt(a) for a in v)
    return f"{v:g}" if isinstance(v, float) else str(v)


class Case:
    def __init__(self, kind, labels, **p):
        self.kind, self.labels, self.p = kind, tuple(labels.split()), p
        self.id = kind + "".join(f"-{k}{_fmt(v)}" for k, v in p.items())

    def __getitem__(self, k):
        return self.p.get(k)

    def gen(self):
        return torch.Generator().manual_seed(zlib.crc32(self.id.encode()))


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _t(inp, dt, *names):
    return [inp[n].detach().to(dt).clone() for n in names]


# ====================================================================================================================== inputs and references
# Every kind has inputs(case) -> {name: fp32 CPU tensor} and ref(case, inputs, dtype) -> {name: tensor of that dtype}: plain torch, run in float64
# and in float32.  Nothing here touches the library or the GPU.

# ---- MoCo ----------------------------------------------------------------------------------------------------------------------------
def _moco_in(c):
    g = c.gen()
    n, k, d = c["N"], c["K"], c["D"]
    kpad = (k + 15) // 16 * 16                                          # as models.moco.MemoryBank pads it
    bank = torch.full((kpad, d), 1e4)                                   # padding rows: large finite garbage that must not leak
    bank[:k] = 0.0 if c["zero_bank"] else F.normalize(_rn(g, k, d), dim=-1)
    s = c["scale"] or 1.0
    return {"q": _rn(g, n, d, scale=s), "k": _rn(g, n, d, scale=s), "bank": bank}


def _moco_ref(c, inp, dt):
    q, k, bank = _t(inp, dt, "q", "k", "bank")
    inv_t = _s(1.0 / c["T"])
    q.requires_grad_(True)
    qn, kn = (F.normalize(q, p=2, dim=-1), F.normalize(k, p=2, dim=-1)) if c["normalize"] else (q * 1.0, k)
    qn.retain_grad()
    pos = (qn * kn).sum(1, keepdim=True) * inv_t
    raw = qn @ bank[:c["K"]].t()
    raw.retain_grad()
    loss = F.cross_entropy(torch.cat((pos, raw * inv_t), 1), torch.zeros(q.shape[0], dtype=torch.long))
    loss.backward()
    return {"loss": loss.detach(), "dneg": raw.grad, "dqn": qn.grad, "dquery": q.grad}


# ---- ReLIC ---------------------------------------------------------------------------------------------------------------------------
def _relic_in(c):
    g = c.gen()
    n, d = c["N"], c["D"]
    s = c["scale"] or 1.0
    out = {nm: _rn(g, n, d, scale=s) for nm in ("zi", "zj", "zo")}
    if c.kind == "relic_kl" and c["normalize"]:                         # the kernel's operands are the unit rows RelicLoss hands it
        out = {nm: F.normalize(t, dim=-1) for nm, t in out.items()}
    out["prior"] = torch.tensor(0.37)
    return out


def _kl_lines(zi, zj, zo, inv_t):
    a = (zi * zo).sum(1) * inv_t                                        # diagonal of zi zo^T
    b = (zj * zo).sum(1) * inv_t
    p, lq = F.softmax(a, -1), F.log_softmax(b, -1)
    return (lq.exp() * (lq - p)).sum()                                  # kl_div(input=p, target=lq, log_target=True, "sum")


def _relic_kl_ref(c, inp, dt):
    zi, zj, zo = (t.requires_grad_(True) for t in _t(inp, dt, "zi", "zj", "zo"))
    term = _s(c["alpha"]) * _kl_lines(zi, zj, zo, _s(1.0 / c["T"]))
    term.backward()
    loss = term.detach() + inp["prior"].to(dt) if c["accumulate"] else term.detach()
    return {"loss": loss, "dzi": zi.grad, "dzj": zj.grad, "dzo": zo.grad}


def _ntxent_lines(zi, zj, normalize, inv_t):
    n = zi.shape[0]
    if normalize:
        zi, zj = F.normalize(zi, p=2, dim=-1), F.normalize(zj, p=2, dim=-1)
    z = torch.cat([zi, zj], dim=0)
    s = (z @ z.t()) * inv_t
    s = s.masked_fill(torch.eye(2 * n, dtype=torch.bool), float("-inf"))
    pos = torch.cat([torch.arange(n, 2 * n), torch.arange(0, n)])
    return (torch.logsumexp(s, dim=1) - s[torch.arange(2 * n), pos]).mean()


def _relic_whole_ref(c, inp, dt):
    zi, zj, zo = (t.requires_grad_(True) for t in _t(inp, dt, "zi", "zj", "zo"))
    inv_t = _s(1.0 / c["T"])
    contrastive = _ntxent_lines(zi, zj, c["normalize"], inv_t)
    ni, nj, no = (F.normalize(t, p=2, dim=-1) for t in (zi, zj, zo)) if c["normalize"] else (zi, zj, zo)
    loss = contrastive + _s(c["alpha"]) * _kl_lines(ni, nj, no, inv_t)
    loss.backward()
    return {"loss": loss.detach(), "dzi": zi.grad, "dzj": zj.grad, "dzo": zo.grad}


# ---- SimSiam / BYOL pair losses ------------------------------------------------------------------------------------------------------
def _pair_in(c):
    g = c.gen()
    b, d = c["shape"]
    out = {nm: _rn(g, b, d) for nm in ("o1", "o2", "t1", "t2")}
    if c.kind == "negdot":                                              # SimSiam's operands are unit rows
        out = {nm: F.normalize(t, dim=-1) for nm, t in out.items()}
    return out


def _negdot_ref(c, inp, dt):
    o1, o2, t1, t2 = _t(inp, dt, "o1", "o2", "t1", "t2")
    scale = _s(0.5 / c["shape"][0])
    return {"loss": -scale * ((o1 * t2).sum() + (o2 * t1).sum()), "do1": -scale * t2, "do2": -scale * t1}


def _mse_ref(c, inp, dt):
    o1, o2, t1, t2 = _t(inp, dt, "o1", "o2", "t1", "t2")
    inv = _s(1.0 / o1.numel())
    a, b = o1 - t2, o2 - t1
    return {"loss": inv * ((a * a).sum() + (b * b).sum()), "do1": (2.0 * inv) * a, "do2": (2.0 * inv) * b}


# ---- Barlow Twins --------------------------------------------------------------------------------------------------------------------
BARLOW_B = 512


def _cgrad_in(c):
    g = c.gen()
    d = c["D"]
    return {"craw": _rn(g, d, d, scale=BARLOW_B ** 0.5) + 0.8 * BARLOW_B * torch.eye(d)}       # B x (a correlation matrix of a half-trained model)


def _cgrad_ref(c, inp, dt):
    (craw,) = _t(inp, dt, "craw")
    inv_b, lam = _s(1.0 / BARLOW_B), _s(0.005)
    eye = torch.eye(c["D"], dtype=dt)
    w = lam * (1 - eye) + eye
    diff = craw * inv_b - eye
    return {"loss": (w * diff * diff).sum(), "G": 2.0 * w * diff * inv_b}


def _barlow_in(c):
    g = c.gen()
    b, d = c["B"], c["D"]
    zi = _rn(g, b, d)
    return {"zi": zi, "zj": 0.7 * zi + 0.7 * _rn(g, b, d)}             # two correlated views


def _barlow_ref(c, inp, dt):
    zi, zj = (t.requires_grad_(True) for t in _t(inp, dt, "zi", "zj"))
    a, b_ = (F.normalize(zi, p=2, dim=-1), F.normalize(zj, p=2, dim=-1)) if c["normalize"] else (zi, zj)
    n, d = zi.shape
    a = (a - a.mean(0)) / a.std(0)
    b_ = (b_ - b_.mean(0)) / b_.std(0)
    cm = (a.t() @ b_) / n
    eye = torch.eye(d, dtype=dt)
    w = _s(0.005) * (1 - eye) + eye
    loss = (w * (cm - eye) ** 2).sum()
    loss.backward()
    return {"loss": loss.detach(), "dzi": zi.grad, "dzj": zj.grad}


# ---- DINO ----------------------------------------------------------------------------------------------------------------------------
def _dino_in(c):
    g = c.gen()
    bs, v, k = c["bs"], c["V"], c["K"]
    s = c["scale"] or 1.0
    return {"teacher": _rn(g, bs, 2, k, scale=s), "student": _rn(g, bs, v, k, scale=s), "center": _rn(g, k, scale=c["centre"] or 0.1),
            "prior": torch.tensor(1.25)}


def _dino_ref(c, inp, dt):
    teacher, student, center = _t(inp, dt, "teacher", "student", "center")
    student.requires_grad_(True)
    temp_s, temp_t, weight = _s(0.1), _s(c["temp_t"]), _s(c["weight"] or 1.0)
    logp = F.log_softmax(student / temp_s, -1)
    total = 0.0
    for g in range(2):
        tgt = F.softmax((teacher[:, g:g + 1, :] - center) / temp_t, -1)
        total = total + (-(tgt * logp).sum(-1).mean())
    term = weight * total
    term.backward()
    loss = term.detach() + inp["prior"].to(dt) if c["accumulate"] else term.detach()
    return {"loss": loss, "dstudent": student.grad}


def _center_in(c):
    g = c.gen()
    k = c["K"]
    return {"center": _rn(g, k, scale=2.0), "t1": _rn(g, c["rows1"], k, scale=3.0) + 1.0, "t2": _rn(g, max(c["rows2"], 1), k, scale=3.0) - 0.5}


def _center_ref(c, inp, dt):
    center, t1, t2 = _t(inp, dt, "center", "t1", "t2")
    m = _s(0.9)
    rows = torch.cat((t1, t2), 0) if c["rows2"] else t1
    return {"center": m * center + (1.0 - m) * rows.mean(0)}


# ---- NT-Xent through SimclrLoss ------------------------------------------------------------------------------------------------------
def _ntxent_in(c):
    g = c.gen()
    n, d = c["N"], c["D"]
    s = c["scale"] or 1.0
    return {"zi": _rn(g, n, d, scale=s), "zj": _rn(g, n, d, scale=s)}


def _ntxent_ref(c, inp, dt):
    zi, zj = (t.requires_grad_(True) for t in _t(inp, dt, "zi", "zj"))
    loss = _ntxent_lines(zi, zj, c["normalize"], _s(1.0 / c["T"]))
    loss.backward()
    return {"loss": loss.detach(), "dzi": zi.grad, "dzj": zj.grad}


# ---- F.normalize ---------------------------------------------------------------------------------------------------------------------
L2_EPS = 1e-12


def _l2_in(c):
    g = c.gen()
    rows, d, ldo = c["shape"]
    z = _rn(g, rows, d, scale=1.7)
    if c["zero_row"] is not None:
        z[c["zero_row"]] = 0.0
    return {"z": z, "dzhat": _rn(g, rows, ldo)}


def _l2_ref(c, inp, dt):
    z, dzhat = _t(inp, dt, "z", "dzhat")
    rows, d, ldo = c["shape"]
    if c["normalize"]:
        inv = 1.0 / z.norm(p=2, dim=-1).clamp_min(_s(L2_EPS))
    else:
        inv = torch.ones(rows, dtype=dt)
    zhat = torch.zeros(rows, ldo, dtype=dt)
    zhat[:, :d] = z * inv[:, None]
    dh, zh = dzhat[:, :d], zhat[:, :d]
    dz = (dh - zh * (zh * dh).sum(1, keepdim=True)) * inv[:, None] if c["normalize"] else dh.clone()
    out = {"zhat": zhat, "dz": dz}
    if c["normalize"]:
        out["inv_norm"] = inv
    if c["zero_row"] is not None:                                       # 1 / eps = 1e12 would drown every other row: that row is checked exactly
        keep = [r for r in range(rows) if r != c["zero_row"]]
        out["dz"], out["inv_norm"] = dz[keep], inv[keep]
    return out


# ---- weight norm ---------------------------------------------------------------------------------------------------------------------
def _wn_in(c):
    g = c.gen()
    rows, cols = c["shape"]
    return {"g": _rn(g, rows) + 2.0, "v": _rn(g, rows, cols, scale=0.3), "dw": _rn(g, rows, cols), "dg0": _rn(g, rows), "dv0": _rn(g, rows, cols)}


def _wn_ref(c, inp, dt):
    g, v, dw, dg0, dv0 = _t(inp, dt, "g", "v", "dw", "dg0", "dv0")
    g.requires_grad_(True)
    v.requires_grad_(True)
    norm = v.norm(dim=1)
    w = v * (g / norm)[:, None]
    (w * dw).sum().backward()
    dg, dv = (g.grad + dg0, v.grad + dv0) if c["accumulate"] else (g.grad, v.grad)
    return {"w": w.detach(), "inv_norm": (1.0 / norm).detach(), "dg": dg, "dv": dv}


# ---- soft-max cross-entropy ----------------------------------------------------------------------------------------------------------
def _ce_in(c):
    g = c.gen()
    n, cl, ld = c["shape"]
    return {"logits": _rn(g, n, ld, scale=3.0), "labels": torch.randint(0, cl, (n,), generator=g, dtype=torch.int32)}


def _ce_ref(c, inp, dt):
    n, cl, ld = c["shape"]
    logits = inp["logits"][:, :cl].to(dt).clone().requires_grad_(True)
    loss = F.cross_entropy(logits, inp["labels"].long())
    loss.backward()
    return {"loss": loss.detach(), "dlogits": logits.grad}


# ---- optimizers ----------------------------------------------------------------------------------------------------------------------
STEPS = 3
SGD_LR, SGD_MOM = 0.2, 0.9


def _opt_in(c):
    g = c.gen()
    n = c["n"]
    gs = 2.0 if c.kind == "adamw" else 0.05
    return {"p": _rn(g, n), "g": _rn(g, STEPS, n, scale=gs), "g2": _rn(g, STEPS, n, scale=gs)}


def _grad(c, inp, dt, step):
    g = inp["g"][step].to(dt)
    return g + inp["g2"][step].to(dt) if c["g2"] else g.clone()


def _sgd_ref(c, inp, dt):
    p = torch.nn.Parameter(inp["p"].to(dt).clone())
    opt = torch.optim.SGD([p], lr=_s(SGD_LR), momentum=_s(SGD_MOM), weight_decay=_s(c["wd"]), nesterov=bool(c["nesterov"]))
    for step in range(STEPS):
        p.grad = _grad(c, inp, dt, step)
        opt.step()
    return {"p": p.detach(), "buf": opt.state[p]["momentum_buffer"]}


ADAM = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-6, wd=0.04)


def _adamw_ref(c, inp, dt):
    p = torch.nn.Parameter(inp["p"].to(dt).clone())
    opt = torch.optim.AdamW([p], lr=_s(ADAM["lr"]), betas=(_s(ADAM["b1"]), _s(ADAM["b2"])), eps=_s(ADAM["eps"]), weight_decay=_s(ADAM["wd"]))
    for step in range(STEPS):
        g = _grad(c, inp, dt, step)
        p.grad = g.clamp(-_s(c["clip"]), _s(c["clip"])) if c["clip"] > 0 else g
        opt.step()
    st = opt.state[p]
    return {"p": p.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}


def _elt_in(c):
    g = c.gen()
    n = c["n"]
    return {"a": _rn(g, n), "b": _rn(g, n), "f": torch.tensor([0.37])}


def _elt_ref(c, inp, dt):
    a, b, f = _t(inp, dt, "a", "b", "f")
    tau = _s(0.996)
    return {"ema": tau * a + (1.0 - tau) * b, "add": a + b, "scale": a * f, "fill": torch.full_like(a, _s(-1.3))}


# ---- MoCo's queue --------------------------------------------------------------------------------------------------------------------
QUEUE_PUSHES = (16, 16, 16, 7, 90)


def _queue_in(c):
    g = c.gen()
    keys = [_rn(g, n, c["D"], scale=2.0) for n in QUEUE_PUSHES]
    keys[1][5] = 0.0                                                    # one all-zero key: F.normalize leaves it zero
    return {f"keys{i}": k for i, k in enumerate(keys)}


def _queue_ref(c, inp, dt):
    bank, ptr = torch.zeros(c["K"], c["D"], dtype=dt), 0
    out = {}
    for i in range(len(QUEUE_PUSHES)):
        for row in inp[f"keys{i}"].to(dt):                              # MemoryBank.add_batch of the reference: row by row
            bank[ptr] = F.normalize(row, dim=-1, p=2)
            ptr = (ptr + 1) % c["K"]
        out[f"bank{i}"] = bank.clone()
    return out


def queue_pointers(k):
    out, ptr = [], 0
    for n in QUEUE_PUSHES:
        ptr = (ptr + n) % k
        out.append(ptr)
    return out


# ====================================================================================================================== the case table
_L2 = "ssv_l2norm_fwd ssv_l2norm_bwd"
_NTX = "ssv_ntxent_fwd_split ssv_ntxent_bwd_split ssv_ntxent_loss ssv_scale " + _L2
KINDS = {
    # kind: (family, entry points reached, both arithmetics, inputs, reference)
    "moco": ("loss-softmax", "ssv_moco_loss_fwd_bwd " + _L2, True, _moco_in, _moco_ref),
    "relic_kl": ("loss-softmax", "ssv_relic_kl_fwd_bwd", False, _relic_in, _relic_kl_ref),
    "relic_whole": ("loss-softmax", "ssv_relic_kl_fwd_bwd " + _NTX, False, _relic_in, _relic_whole_ref),
    "negdot": ("loss-elementwise", "ssv_negdot_pair_fwd_bwd", False, _pair_in, _negdot_ref),
    "mse": ("loss-elementwise", "ssv_mse_pair_fwd_bwd", False, _pair_in, _mse_ref),
    "cgrad": ("loss-elementwise", "ssv_barlow_cgrad", False, _cgrad_in, _cgrad_ref),
    "barlow": ("loss-elementwise", "ssv_barlow_cgrad ssv_scale ssv_fill " + _L2, True, _barlow_in, _barlow_ref),
    "dino": ("loss-softmax", "ssv_dino_loss", False, _dino_in, _dino_ref),
    "center": ("loss-elementwise", "ssv_dino_center_update", False, _center_in, _center_ref),
    "ntxent": ("loss-softmax", _NTX, False, _ntxent_in, _ntxent_ref),
    "ntxent_wide": ("loss-softmax", "ssv_ntxent_gram_fwd ssv_ntxent_gram_weights ssv_ntxent_loss ssv_scale ssv_fill " + _L2, True, _ntxent_in, _ntxent_ref),
    "l2norm": ("normalisation", _L2, False, _l2_in, _l2_ref),
    "wn": ("normalisation", "ssv_weightnorm_fwd ssv_weightnorm_bwd", False, _wn_in, _wn_ref),
    "ce": ("loss-softmax", "ssv_softmax_ce_fwd_bwd", False, _ce_in, _ce_ref),
    "sgdn": ("optimizer", "ssv_sgd_nesterov ssv_sgd_nesterov_dev", False, _opt_in, _sgd_ref),
    "sgd": ("optimizer", "ssv_sgd", False, _opt_in, _sgd_ref),
    "adamw": ("optimizer", "ssv_adamw ssv_adamw_counted ssv_adamw_counted_dev", False, _opt_in, _adamw_ref),
    "elt": ("optimizer", "ssv_ema ssv_add ssv_scale ssv_fill", False, _elt_in, _elt_ref),
    "queue": ("normalisation", "ssv_queue_push ssv_queue_push_counted", False, _queue_in, _queue_ref),
}

CASES = [
    # ---- MoCo: (N, K, D, T, normalize)
    Case("moco", "moco.config", N=256, K=1000, D=128, T=0.07, normalize=True),
    Case("moco", "moco.tiny", N=9, K=50, D=32, T=0.07, normalize=True),
    Case("moco", "moco.ragged_pad", N=33, K=4099, D=200, T=0.07, normalize=True),
    Case("moco", "moco.d_trips moco.ragged_pad", N=17, K=300, D=320, T=0.2, normalize=True),
    Case("moco", "moco.k65536", N=64, K=65536, D=128, T=0.07, normalize=True),
    Case("moco", "moco.unnormalised moco.ragged_pad", N=37, K=300, D=128, T=1.0, normalize=False, scale=6.0),
    Case("moco", "moco.zero_bank moco.ragged_pad", N=256, K=1000, D=128, T=0.07, normalize=True, zero_bank=True),
    # ---- ReLIC: the invariance term alone, accumulate_loss 0 and 1 ...
    Case("relic_kl", "relic.config", N=512, D=128, T=1.0, alpha=0.5, normalize=True),
    Case("relic_kl", "relic.config relic.accumulate", N=512, D=128, T=1.0, alpha=0.5, normalize=True, accumulate=True),
    Case("relic_kl", "relic.tiny", N=10, D=32, T=1.0, alpha=0.5, normalize=True),
    Case("relic_kl", "relic.n_trips", N=1500, D=128, T=0.1, alpha=0.5, normalize=True),
    Case("relic_kl", "relic.n_trips relic.accumulate", N=4096, D=128, T=1.0, alpha=0.5, normalize=True, accumulate=True),
    Case("relic_kl", "relic.n_trips", N=4096, D=128, T=1.0, alpha=0.5, normalize=True),
    Case("relic_kl", "relic.ragged", N=13, D=100, T=1.0, alpha=0.5, normalize=False, scale=0.3),
    Case("relic_kl", "relic.ragged relic.accumulate", N=13, D=100, T=1.0, alpha=0.5, normalize=False, scale=0.3, accumulate=True),
    # ... and RelicLoss as a whole
    Case("relic_whole", "relic.whole relic.config", N=512, D=128, T=1.0, alpha=0.5, normalize=True),
    Case("relic_whole", "relic.whole relic.tiny", N=10, D=32, T=1.0, alpha=0.5, normalize=True),
    Case("relic_whole", "relic.whole relic.n_trips", N=1500, D=128, T=0.1, alpha=0.5, normalize=True),
    Case("relic_whole", "relic.whole relic.n_trips", N=4096, D=128, T=1.0, alpha=0.5, normalize=True),
    Case("relic_whole", "relic.whole relic.ragged", N=13, D=100, T=1.0, alpha=0.5, normalize=False, scale=0.3),
    # ---- SimSiam / BYOL pair losses
    Case("negdot", "negdot.small", shape=(12, 64)),
    Case("negdot", "negdot.small", shape=(7, 33)),
    Case("negdot", "negdot.blocks", shape=(512, 1024)),
    Case("negdot", "negdot.stride", shape=(512, 4096)),
    Case("mse", "mse.small", shape=(16, 128)),
    Case("mse", "mse.small", shape=(7, 33)),
    Case("mse", "mse.blocks", shape=(512, 128)),
    Case("mse", "mse.stride", shape=(512, 4096)),
    # ---- Barlow Twins
    Case("cgrad", "barlow.cgrad_min", D=16),
    Case("cgrad", "barlow.cgrad_min", D=48),
    Case("cgrad", "barlow.cgrad", D=128),
    Case("cgrad", "barlow.cgrad", D=1000),
    Case("cgrad", "barlow.cgrad_stride", D=4096),
    Case("barlow", "barlow.whole", B=512, D=128, normalize=True),
    Case("barlow", "barlow.whole", B=33, D=48, normalize=True),
    Case("barlow", "barlow.whole", B=1024, D=2048, normalize=True),
    Case("barlow", "barlow.whole", B=128, D=4096, normalize=False),
    # ---- DINO: (bs, V, K, input scale), teacher temperatures 0.04 and 0.07
    Case("dino", "dino.config", bs=64, V=8, K=1024, scale=1.0, temp_t=0.04),
    Case("dino", "dino.config dino.centre dino.weight_acc", bs=64, V=8, K=1024, scale=1.0, temp_t=0.07, centre=5.0, weight=0.5, accumulate=True),
    Case("dino", "dino.config", bs=6, V=10, K=1024, scale=3.0, temp_t=0.07),
    Case("dino", "dino.k65536", bs=3, V=8, K=65536, scale=1.0, temp_t=0.04),
    Case("dino", "dino.k65536 dino.centre", bs=3, V=8, K=65536, scale=1.0, temp_t=0.07, centre=5.0),
    Case("dino", "dino.v2 dino.k_ragged", bs=5, V=2, K=1000, scale=8.0, temp_t=0.04),
    Case("dino", "dino.v2 dino.k_ragged dino.weight_acc", bs=5, V=2, K=1000, scale=8.0, temp_t=0.07, weight=1.7, accumulate=True),
    Case("dino", "dino.k_ragged", bs=2, V=3, K=257, scale=1.0, temp_t=0.04),
    Case("dino", "dino.k_ragged dino.centre", bs=2, V=3, K=257, scale=1.0, temp_t=0.07, centre=5.0),
    Case("dino", "dino.k64", bs=2, V=3, K=64, scale=1.0, temp_t=0.04),
    Case("center", "dino.center_one", K=257, rows1=6, rows2=0),
    Case("center", "dino.center_two", K=257, rows1=6, rows2=6),
    Case("center", "dino.center_one", K=65536, rows1=3, rows2=0),
    Case("center", "dino.center_two", K=65536, rows1=3, rows2=5),
    # ---- NT-Xent where the other tests stop
    Case("ntxent", "ntxent.online_max", N=64, D=128, T=1.0, normalize=False, scale=4.0),
    Case("ntxent", "ntxent.online_max ntxent.padded", N=100, D=96, T=0.2, normalize=False, scale=2.0),
    Case("ntxent", "ntxent.padded", N=40, D=70, T=0.5, normalize=True),
    Case("ntxent", "ntxent.padded", N=40, D=70, T=1.0, normalize=False),
    Case("ntxent", "ntxent.padded", N=40, D=20, T=0.2, normalize=True),
    Case("ntxent_wide", "ntxent.wide", N=48, D=512, T=1.0, normalize=False, scale=1.5),
    # ---- F.normalize: (rows, D, ldo)
    Case("l2norm", "l2norm.ragged", shape=(37, 100, 128), normalize=True),
    Case("l2norm", "l2norm.small_d", shape=(5, 20, 32), normalize=True),
    Case("l2norm", "l2norm.wide", shape=(258, 4096, 4096), normalize=True),
    Case("l2norm", "l2norm.zero_row", shape=(3, 128, 128), normalize=True, zero_row=1),
    Case("l2norm", "l2norm.copy_padded", shape=(37, 100, 128), normalize=False),
    Case("l2norm", "l2norm.copy_padded l2norm.small_d", shape=(5, 20, 32), normalize=False),
    # ---- weight norm
    Case("wn", "wn.config wn.overwrite", shape=(1024, 512), accumulate=False),
    Case("wn", "wn.config wn.accumulate", shape=(1024, 512), accumulate=True),
    Case("wn", "wn.ragged wn.overwrite", shape=(1023, 130), accumulate=False),
    Case("wn", "wn.ragged wn.accumulate", shape=(1023, 130), accumulate=True),
    Case("wn", "wn.ragged wn.overwrite", shape=(5, 63), accumulate=False),
    Case("wn", "wn.ragged wn.accumulate", shape=(5, 63), accumulate=True),
    # ---- soft-max cross-entropy: (N, C, ld)
    Case("ce", "ce.small", shape=(37, 10, 12)),
    Case("ce", "ce.small", shape=(256, 10, 12)),
    Case("ce", "ce.c_trips ce.ragged_rows", shape=(129, 1000, 1000)),
    Case("ce", "ce.c_trips", shape=(3, 700, 704)),
]
for _n in (5, 1001, 4099, BIG):
    _big = " sgdn.stride" if _n == BIG else ""
    CASES += [
        Case("sgdn", "sgdn.tail sgdn.dev_bitwise" + _big, n=_n, wd=1e-4, nesterov=True, g2=False),
        Case("sgdn", "sgdn.tail_g2 sgdn.dev_bitwise" + _big, n=_n, wd=1e-4, nesterov=True, g2=True),
        Case("sgd", "sgd.plain" + (" sgd.stride" if _n == BIG else ""), n=_n, wd=(0.0 if _n in (5, 4099) else 5e-4), nesterov=False),
        Case("sgd", "sgd.nesterov" + (" sgd.stride" if _n == BIG else ""), n=_n, wd=(5e-4 if _n in (5, 4099) else 0.0), nesterov=True),
        Case("adamw", "adamw.g2 adamw.clip0 adamw.counted adamw.counted_dev", n=_n, g2=True, clip=0.0),
        Case("adamw", "adamw.g2 adamw.clip3 adamw.counted adamw.counted_dev", n=_n, g2=True, clip=3.0),
        Case("adamw", "adamw.clip3 adamw.counted adamw.counted_dev", n=_n, g2=False, clip=3.0),
        Case("elt", "elt.ema elt.add elt.scale elt.fill", n=_n),
    ]
CASES += [
    Case("queue", "queue.counted queue.wrap queue.n_gt_k", K=40, D=100),
    Case("queue", "queue.counted queue.wrap queue.n_gt_k", K=40, D=128),
]

# extern "C" entry points of the four files that this file leaves to another test, each with its reason
EXCLUDED = {
    "ssv_ntxent_fwd": "the split entry with splits = 1; ops always calls ssv_ntxent_fwd_split, and tests/test_gpu_config3.py compares the two forms",
    "ssv_ntxent_bwd": "the split entry with splits = 1 (as above)",
}
# entry points outside the four files that the table names
EXTRA = {
    "ssv_softmax_ce_fwd_bwd": "evalknn.hip: the linear probe's loss",
    "ssv_fill": "runtime.hip: the element-wise helper next to ssv_add / ssv_scale",
}


# ====================================================================================================================== GPU-free honesty tests
def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(\S+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def launching_entry_points():
    """extern "C" functions of loss.hip, siblings.hip, dino.hip and optim.hip that return a status (the size_t / int64_t ones are workspace and
    split-count queries: they launch nothing)."""
    out = set()
    for name in ("loss.hip", "siblings.hip", "dino.hip", "optim.hip"):
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        out |= set(re.findall(r'^extern "C" int (ssv_\w+)\(', src, flags=re.M))
    return out


def test_case_table_names_every_entry_point():
    """GPU-free: the entry points named by CASES are exactly the status-returning extern "C" functions of the four files, minus EXCLUDED, plus EXTRA."""
    named = {e for c in CASES for e in KINDS[c.kind][1].split()}
    have = launching_entry_points()
    assert len(have) >= 28
    assert set(EXCLUDED) <= have, "EXCLUDED names something the sources no longer have"
    assert not set(EXTRA) & have
    assert named == (have - set(EXCLUDED)) | set(EXTRA), f"missing {sorted(((have - set(EXCLUDED)) | set(EXTRA)) - named)}, stray {sorted(named - have - set(EXTRA))}"


def test_case_table_covers_every_documented_branch():
    """GPU-free: every branch label of the docstring has a case, every label of a case is documented, the documented entry point is one the case's
    kind reaches (or the loss module that composes them), ids are unique, no family is missing its FACTOR / FLOOR, and the bounds respect their caps."""
    doc = documented_labels()
    assert len(doc) >= 60
    used = {b for c in CASES for b in c.labels}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    for c in CASES:
        for b in c.labels:
            assert doc[b] in KINDS[c.kind][1].split() or doc[b].endswith("Loss"), (c.id, b)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    fams = {KINDS[c.kind][0] for c in CASES}
    assert fams == set(FACTOR) == set(FLOOR) and len(fams) == 4
    assert all(1.0 <= f <= 8.0 and math.log2(f).is_integer() for f in FACTOR.values())
    assert all(0.0 <= f <= 16 * U for f in FLOOR.values())


def _err(x, ref64):
    d = x.detach().double().cpu() - ref64
    return float(d.norm() / ref64.norm().clamp_min(1e-300)), float(d.abs().max() / ref64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_is_well_conditioned(case):
    """GPU-free, condition (b): the fp64 reference is finite and the fp32 evaluation of the same lines is within 1e-3 of it (e and m), for every
    tensor of every case - all sizes included (the whole table takes well under a minute of CPU time)."""
    fam, _, _, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    assert set(r64) == set(r32)
    for name, t in r64.items():
        assert t.dtype == torch.float64 and r32[name].dtype == torch.float32, name
        assert torch.isfinite(t).all() and torch.isfinite(r32[name]).all(), name
        assert float(t.abs().max()) > 0, f"{name}: the reference is identically zero"
        e, m = _err(r32[name], t)
        print(f"{case.id} {name}: e(ref32) {e:.3e} m(ref32) {m:.3e}")
        assert e <= COND and m <= COND, f"{name}: ref32 is {e:.2e} / {m:.2e} from ref64 - the case measures nothing"


# ====================================================================================================================== GPU side
def _lib():
    from ssv_amd import _lib as L
    return L


def _ratio(got, ref, floor):
    if got <= floor:
        return 0.0
    return (got - floor) / ref if ref > 0 else float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib().load()
    yield torch.device("cuda:0")
    path = os.environ.get("SSV_LOSS_REPORT")
    if path:
        fams = {}
        for cid, tensors in REPORT.items():
            fam = tensors["family"]
            f = fams.setdefault(fam, {"FACTOR": FACTOR[fam], "FLOOR": FLOOR[fam], "worst_e_ratio": 0.0, "worst_m_ratio": 0.0, "worst_e_case": "", "worst_m_case": ""})
            for name, r in tensors.items():
                if name == "family":
                    continue
                for k in ("e", "m"):
                    ratio = _ratio(r[f"{k}_got"], r[f"{k}_ref32"], FLOOR[fam])
                    if ratio > f[f"worst_{k}_ratio"]:
                        f[f"worst_{k}_ratio"], f[f"worst_{k}_case"] = ratio, f"{cid} {name}"
        with open(path, "w") as fh:
            json.dump({"families": fams, "cases": REPORT}, fh, indent=1, sort_keys=True)


class Ctx:
    """The device side of one run of one case: uploaded inputs (kept to prove them untouched), guarded outputs, stated identities."""

    def __init__(self, dev):
        self.dev, self.ins, self.bufs, self.same = dev, [], [], []

    def up(self, name, t, overwritten=False):
        d = t.to(self.dev).contiguous()
        if not overwritten:
            self.ins.append((name, d, d.clone()))
        return d

    def out(self, name, shape, prior=None, nan_ok=False):
        n = math.prod(shape)
        buf = torch.full((n + GUARD,), float("nan"), device=self.dev)
        if prior is not None:
            buf[:n].copy_(prior.reshape(-1))
        self.bufs.append((name, buf, n, nan_ok))
        return buf[:n].view(shape)

    def ws(self, name, nbytes):
        """a guarded workspace of the size the library asks for: (tensor, bytes)"""
        nbytes = int(nbytes)
        n = (nbytes + 3) // 4
        buf = torch.full((n + GUARD,), float("nan"), device=self.dev)
        self.bufs.append((name, buf, n, True))
        return buf, nbytes

    def ints(self, name, values, dtype):
        """a guarded integer output: 64 sentinels behind it"""
        buf = torch.full((len(values) + 64,), -77, dtype=dtype, device=self.dev)
        buf[:len(values)] = torch.tensor(values, dtype=dtype)
        self.bufs.append((name, buf, len(values), False))
        return buf[:len(values)]

    def verify(self, what):
        torch.cuda.synchronize()
        for name, d, keep in self.ins:
            assert torch.equal(d, keep), f"{what}: input {name} was modified"
        for name, buf, n, nan_ok in self.bufs:
            if buf.is_floating_point():
                assert nan_ok or not torch.isnan(buf[:n]).any(), f"{what} {name}: {int(torch.isnan(buf[:n]).sum())} elements never written (or NaN)"
                assert torch.isnan(buf[n:]).all(), f"{what} {name}: wrote past its end"
            else:
                assert (buf[n:] == -77).all(), f"{what} {name}: wrote past its end"
        for name, a, b in self.same:
            assert a.shape == b.shape and torch.equal(a, b), f"{what}: {name} not bit-identical (max |diff| {float((a.double() - b.double()).abs().max()):.3e})"


def _module_run(loss_fn, *xs):
    xs = [x.clone().requires_grad_(True) for x in xs]
    loss = loss_fn(*xs)
    loss.backward()
    return loss.detach().reshape(1), [x.grad for x in xs]


# ---- the runners: (case, inputs, ctx) -> {name: device tensor}; exact statements are asserted inside -------------------------------------
def _moco_gpu(c, inp, ctx):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    L = _lib()
    P = L.ptr
    n, k, d = c["N"], c["K"], c["D"]
    q, kk, bank = ctx.up("q", inp["q"]), ctx.up("k", inp["k"]), ctx.up("bank", inp["bank"])
    ldk = bank.shape[0]
    norm = bool(c["normalize"])
    inv_t = 1.0 / float(c["T"])
    ops.invalidate_weight_caches()
    qn, inv_q = ops.l2norm_fwd(q, norm)
    kn, _ = ops.l2norm_fwd(kk, norm)
    neg0 = ops.conv2d_fwd(qn.view(n, 1, 1, d), bank).view(n, ldk)      # [N, K_pad] products with the queue (MFMA GEMM)
    neg = ctx.out("neg", (n, ldk), prior=neg0)
    loss, dq = ctx.out("loss", (1,)), ctx.out("dq", (n, d))
    ws, wsb = ctx.ws("workspace", n * 8)
    L.call("ssv_moco_loss_fwd_bwd", n, d, k, ldk, P(qn), P(kn), P(neg), inv_t, P(loss), P(dq), P(ws), wsb, L.stream())
    dneg = neg[:, :k].clone()
    assert ldk == k or bool((neg[:, k:] == 0).all()), "neg[:, K:ldk] is not exactly zero"
    ops.conv2d_dgrad(neg.view(n, 1, 1, -1), bank, (n, 1, 1, d), addend=dq.view(n, 1, 1, d), out=dq.view(n, 1, 1, d))   # dq += P . bank
    dqn = dq.clone()
    dquery = ops.l2norm_bwd(qn, inv_q, dq, d, norm)
    mloss, (mgrad,) = _module_run(lambda x: losses.MocoLoss(norm, c["T"])(x, kk, bank, k), q)
    ctx.same += [("MocoLoss loss vs the composition", mloss, loss), ("MocoLoss gradient vs the composition", mgrad, dquery)]
    return {"loss": loss, "dneg": dneg, "dqn": dqn, "dquery": dquery}


def _relic_kl_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, d = c["N"], c["D"]
    zi, zj, zo = (ctx.up(nm, inp[nm]) for nm in ("zi", "zj", "zo"))
    inv_t, alpha, acc = 1.0 / float(c["T"]), float(c["alpha"]), bool(c["accumulate"])

    def run(prior, accumulate):
        loss = ctx.out("loss", (1,), prior=prior)
        outs = [ctx.out(nm, (n, d)) for nm in ("dzi", "dzj", "dzo")]
        ws, wsb = ctx.ws("workspace", L.load().ssv_relic_kl_workspace_bytes(n))
        L.call("ssv_relic_kl_fwd_bwd", n, d, P(zi), P(zj), P(zo), inv_t, alpha, P(loss), int(accumulate), *(P(o) for o in outs), P(ws), wsb, L.stream())
        return [loss] + outs
    prior = inp["prior"].reshape(1) if acc else None
    got, again = run(prior, acc), run(prior, acc)
    ctx.same += [(f"second call, output {i}", a, b) for i, (a, b) in enumerate(zip(got, again))]
    zero, plain = run(torch.zeros(1), True), run(None, False)
    ctx.same += [(f"accumulate on a zero prior vs overwrite, output {i}", a, b) for i, (a, b) in enumerate(zip(zero, plain))]
    return dict(zip(("loss", "dzi", "dzj", "dzo"), got))


def _relic_whole_gpu(c, inp, ctx):
    from ssv_amd.utils import losses
    zs = [ctx.up(nm, inp[nm]) for nm in ("zi", "zj", "zo")]
    fn = losses.RelicLoss(bool(c["normalize"]), c["T"], c["alpha"])
    loss, grads = _module_run(fn, *zs)
    loss2, grads2 = _module_run(fn, *zs)
    ctx.same += [("second call, loss", loss, loss2)] + [(f"second call, gradient {i}", a, b) for i, (a, b) in enumerate(zip(grads, grads2))]
    return dict(zip(("loss", "dzi", "dzj", "dzo"), [loss] + grads))


def _pair_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    o1, o2, t1, t2 = (ctx.up(nm, inp[nm]) for nm in ("o1", "o2", "t1", "t2"))
    n = o1.numel()
    entry, scale = ("ssv_negdot_pair_fwd_bwd", 0.5 / c["shape"][0]) if c.kind == "negdot" else ("ssv_mse_pair_fwd_bwd", 1.0 / n)

    def run():
        loss, do1, do2 = ctx.out("loss", (1,)), ctx.out("do1", o1.shape), ctx.out("do2", o2.shape)
        ws, wsb = ctx.ws("workspace", L.load().ssv_reduce_workspace_bytes(n))
        L.call(entry, n, P(o1), P(o2), P(t1), P(t2), scale, P(loss), P(do1), P(do2), P(ws), wsb, L.stream())
        return loss, do1, do2
    got, again = run(), run()
    ctx.same += [(f"second call, output {i}", a, b) for i, (a, b) in enumerate(zip(got, again))]
    return dict(zip(("loss", "do1", "do2"), got))


def _cgrad_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    d = c["D"]
    craw = ctx.up("craw", inp["craw"])

    def run():
        loss, g = ctx.out("loss", (1,)), ctx.out("G", (d, d))
        ws, wsb = ctx.ws("workspace", L.load().ssv_reduce_workspace_bytes(d * d))
        L.call("ssv_barlow_cgrad", d, P(craw), 1.0 / BARLOW_B, 0.005, P(loss), P(g), P(ws), wsb, L.stream())
        return loss, g
    got, again = run(), run()
    ctx.same += [(f"second call, output {i}", a, b) for i, (a, b) in enumerate(zip(got, again))]
    return dict(zip(("loss", "G"), got))


def _barlow_gpu(c, inp, ctx):
    from ssv_amd.utils import losses
    zi, zj = ctx.up("zi", inp["zi"]), ctx.up("zj", inp["zj"])
    loss, grads = _module_run(losses.BarlowLoss(bool(c["normalize"]), 0.005), zi, zj)
    return {"loss": loss, "dzi": grads[0], "dzj": grads[1]}


def _dino_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    bs, v, k = c["bs"], c["V"], c["K"]
    teacher, student, center = (ctx.up(nm, inp[nm]) for nm in ("teacher", "student", "center"))
    weight, acc = float(c["weight"] or 1.0), bool(c["accumulate"])

    def run(prior, accumulate):
        loss, ds = ctx.out("loss", (1,), prior=prior), ctx.out("dstudent", (bs, v, k))
        ws, wsb = ctx.ws("workspace", L.load().ssv_dino_loss_workspace_bytes(bs, v, k))
        L.call("ssv_dino_loss", bs, v, k, P(teacher), P(student), P(center), 0.1, float(c["temp_t"]), weight, P(loss), int(accumulate), P(ds), P(ws), wsb, L.stream())
        return loss, ds
    prior = inp["prior"].reshape(1) if acc else None
    got, again = run(prior, acc), run(prior, acc)
    zero, plain = run(torch.zeros(1), True), run(None, False)
    for i in range(2):
        ctx.same += [(f"second call, output {i}", got[i], again[i]), (f"accumulate on a zero prior vs overwrite, output {i}", zero[i], plain[i])]
    return {"loss": got[0], "dstudent": got[1]}


def _center_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    k = c["K"]
    t1, t2 = ctx.up("t1", inp["t1"]), ctx.up("t2", inp["t2"])
    center = ctx.out("center", (k,), prior=inp["center"])
    L.call("ssv_dino_center_update", k, c["rows1"], P(t1), c["rows2"], P(t2) if c["rows2"] else None, 0.9, P(center), L.stream())
    return {"center": center}


def _ntxent_gpu(c, inp, ctx):
    from ssv_amd.utils import losses
    zi, zj = ctx.up("zi", inp["zi"]), ctx.up("zj", inp["zj"])
    fn = losses.SimclrLoss(bool(c["normalize"]), c["T"])
    loss, grads = _module_run(fn, zi, zj)
    loss2, grads2 = _module_run(fn, zi, zj)
    ctx.same += [("second call, loss", loss, loss2), ("second call, dzi", grads[0], grads2[0]), ("second call, dzj", grads[1], grads2[1])]
    return {"loss": loss, "dzi": grads[0], "dzj": grads[1]}


def _l2_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    rows, d, ldo = c["shape"]
    norm = int(bool(c["normalize"]))
    z, dzhat = ctx.up("z", inp["z"]), ctx.up("dzhat", inp["dzhat"])
    zhat, dz = ctx.out("zhat", (rows, ldo)), ctx.out("dz", (rows, d))
    inv = ctx.out("inv_norm", (rows,)) if norm else None
    L.call("ssv_l2norm_fwd", rows, d, P(z), norm, L2_EPS, P(zhat), ldo, P(inv), L.stream())
    L.call("ssv_l2norm_bwd", rows, d, P(zhat), ldo, P(inv), P(dzhat), ldo, norm, P(dz), L.stream())
    assert d == ldo or bool((zhat[:, d:] == 0).all()), "padding columns of zhat are not zero"
    out = {"zhat": zhat, "dz": dz}
    if norm:
        out["inv_norm"] = inv
    else:
        ctx.same += [("normalize = 0: zhat is a copy", zhat[:, :d], z), ("normalize = 0: dz is a copy", dz, dzhat[:, :d])]
    r = c["zero_row"]
    if r is not None:
        eps = torch.tensor(L2_EPS, dtype=torch.float32)
        assert bool((zhat[r] == 0).all()), "an all-zero row must stay zero"
        assert float(inv[r]) == float(1.0 / eps), f"inv_norm of an all-zero row is {float(inv[r])}, not 1 / eps"
        assert torch.isfinite(zhat).all()
        ctx.same.append(("dz of the all-zero row = dzhat / eps", dz[r], dzhat[r, :d] * (1.0 / eps).to(ctx.dev)))
        keep = [i for i in range(rows) if i != r]
        out["dz"], out["inv_norm"] = dz[keep], inv[keep]
    return out


def _wn_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    rows, cols = c["shape"]
    acc = bool(c["accumulate"])
    g, v, dw = ctx.up("g", inp["g"]), ctx.up("v", inp["v"]), ctx.up("dw", inp["dw"])
    w, inv = ctx.out("w", (rows, cols)), ctx.out("inv_norm", (rows,))
    L.call("ssv_weightnorm_fwd", rows, cols, P(g), P(v), P(w), P(inv), L.stream())

    def bwd(dg0, dv0, accumulate):
        dg, dv = ctx.out("dg", (rows,), prior=dg0), ctx.out("dv", (rows, cols), prior=dv0)
        L.call("ssv_weightnorm_bwd", rows, cols, P(dw), P(g), P(v), P(inv), P(dg), P(dv), int(accumulate), L.stream())
        return dg, dv
    dg, dv = bwd(inp["dg0"], inp["dv0"], True) if acc else bwd(None, None, False)
    zero, plain = bwd(torch.zeros(rows), torch.zeros(rows, cols), True), bwd(None, None, False)
    ctx.same += [("dg: accumulate on a zero prior vs overwrite", zero[0], plain[0]), ("dv: accumulate on a zero prior vs overwrite", zero[1], plain[1])]
    return {"w": w, "inv_norm": inv, "dg": dg, "dv": dv}


def _ce_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, cl, ld = c["shape"]
    logits, labels = ctx.up("logits", inp["logits"]), ctx.up("labels", inp["labels"])

    def run():
        stats, dl = ctx.out("stats", (2,)), ctx.out("dlogits", (n, ld))
        ws, wsb = ctx.ws("workspace", L.load().ssv_softmax_ce_workspace_bytes(n))
        L.call("ssv_softmax_ce_fwd_bwd", n, cl, ld, P(logits), P(labels), P(stats), P(dl), P(ws), wsb, L.stream())
        return stats, dl
    (stats, dl), again = run(), run()
    ctx.same += [("second call, stats", stats, again[0]), ("second call, dlogits", dl, again[1])]
    assert ld == cl or bool((dl[:, cl:] == 0).all()), "padding columns of dlogits are not zero"
    acc = float((inp["logits"][:, :cl].argmax(1) == inp["labels"].long()).float().mean())
    assert abs(float(stats[1]) - acc) <= 1e-6, f"accuracy {float(stats[1])} vs {acc}"
    return {"loss": stats[:1], "dlogits": dl[:, :cl]}


def _sgd_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n = c["n"]
    gs = [ctx.up(f"g[{s}]", inp["g"][s]) for s in range(STEPS)]
    g2 = [ctx.up(f"g2[{s}]", inp["g2"][s]) for s in range(STEPS)] if c["g2"] else [None] * STEPS
    p, buf = ctx.out("p", (n,), prior=inp["p"]), ctx.out("buf", (n,))
    lr, wd, mom = SGD_LR, float(c["wd"]), SGD_MOM
    if c.kind == "sgd":
        for s in range(STEPS):
            L.call("ssv_sgd", n, P(p), P(gs[s]), P(buf), lr, wd, mom, int(bool(c["nesterov"])), int(s == 0), L.stream())
        return {"p": p, "buf": buf}
    pd, bufd = ctx.out("p (device hyper-parameters)", (n,), prior=inp["p"]), ctx.out("buf (device hyper-parameters)", (n,))
    hyper = ctx.up("hyper", torch.tensor([lr, wd, mom, 1.0]), overwritten=True)
    for s in range(STEPS):
        hyper[3] = 1.0 if s == 0 else 0.0
        L.call("ssv_sgd_nesterov", n, P(p), P(gs[s]), P(g2[s]), P(buf), lr, wd, mom, int(s == 0), L.stream())
        L.call("ssv_sgd_nesterov_dev", n, P(pd), P(gs[s]), P(g2[s]), P(bufd), P(hyper), L.stream())
    ctx.same += [("ssv_sgd_nesterov_dev vs ssv_sgd_nesterov: p", pd, p), ("ssv_sgd_nesterov_dev vs ssv_sgd_nesterov: buf", bufd, buf)]
    return {"p": p, "buf": buf}


def _adamw_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n, clip = c["n"], float(c["clip"])
    a = ADAM
    gs = [ctx.up(f"g[{s}]", inp["g"][s]) for s in range(STEPS)]
    g2 = [ctx.up(f"g2[{s}]", inp["g2"][s]) for s in range(STEPS)] if c["g2"] else [None] * STEPS
    zero = torch.zeros(n)
    sets = [[ctx.out(f"{nm} ({form})", (n,), prior=pr) for nm, pr in (("p", inp["p"]), ("m", zero), ("v", zero))] for form in ("host", "counted", "counted_dev")]
    step_c, step_d = ctx.ints("step (counted)", [0], torch.int64), ctx.ints("step (counted_dev)", [0], torch.int64)
    bc_c, bc_d = ctx.out("bc (counted)", (4,), nan_ok=True), ctx.out("bc (counted_dev)", (4,), prior=torch.tensor([0.0, 0.0, a["lr"], a["wd"]]))
    for s in range(STEPS):
        (p, m, v), (pc, mc, vc), (pd, md, vd) = sets
        L.call("ssv_adamw", n, P(p), P(gs[s]), P(g2[s]), P(m), P(v), a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], s + 1, clip, L.stream())
        L.call("ssv_adamw_counted", n, P(pc), P(gs[s]), P(g2[s]), P(mc), P(vc), a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], P(step_c), P(bc_c), clip, L.stream())
        L.call("ssv_adamw_counted_dev", n, P(pd), P(gs[s]), P(g2[s]), P(md), P(vd), a["b1"], a["b2"], a["eps"], P(step_d), P(bc_d), clip, L.stream())
        assert int(step_c) == s + 1 and int(step_d) == s + 1, f"device step counters {int(step_c)}, {int(step_d)} after {s + 1} calls"
    for form, other in (("ssv_adamw_counted", sets[1]), ("ssv_adamw_counted_dev", sets[2])):
        ctx.same += [(f"{form} vs ssv_adamw: {nm}", o, h) for nm, o, h in zip("pmv", other, sets[0])]
    return dict(zip(("p", "m", "v"), sets[0]))


def _elt_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n = c["n"]
    a, b, f = ctx.up("a", inp["a"]), ctx.up("b", inp["b"]), ctx.up("f", inp["f"])
    ema, add, scale, fill = (ctx.out(nm, (n,), prior=inp["a"]) for nm in ("ema", "add", "scale", "fill"))
    L.call("ssv_ema", n, P(ema), P(b), 0.996, L.stream())
    L.call("ssv_add", n, P(add), P(b), L.stream())
    L.call("ssv_scale", n, P(scale), P(f), L.stream())
    L.call("ssv_fill", n, P(fill), -1.3, L.stream())
    exact = _elt_ref(c, inp, torch.float32)                             # one correctly rounded operation per element: the same bits as the CPU's
    ctx.same += [(f"{nm} is exact", got, exact[nm].to(ctx.dev)) for nm, got in (("add", add), ("scale", scale), ("fill", fill))]
    return {"ema": ema, "add": add, "scale": scale, "fill": fill}


def _queue_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    k, d = c["K"], c["D"]
    kpad = (k + 15) // 16 * 16
    prior = torch.zeros(kpad, d)
    prior[k:] = 7.0                                                     # rows >= K: never touched
    bank, bank_c = ctx.out("bank", (kpad, d), prior=prior), ctx.out("bank (counted)", (kpad, d), prior=prior)
    ptr_dev = ctx.ints("queue pointer", [0], torch.int32)
    out, ptr = {}, 0
    for i, (n, want) in enumerate(zip(QUEUE_PUSHES, queue_pointers(k))):
        keys = ctx.up(f"keys{i}", inp[f"keys{i}"])
        L.call("ssv_queue_push", k, d, P(bank), ptr, n, P(keys), L2_EPS, L.stream())
        L.call("ssv_queue_push_counted", k, d, P(bank_c), P(ptr_dev), n, P(keys), L2_EPS, L.stream())
        ptr = (ptr + n) % k
        assert ptr == want and int(ptr_dev) == want, f"push {i}: device pointer {int(ptr_dev)}, expected {want}"
        assert torch.equal(bank, bank_c), f"push {i}: ssv_queue_push_counted differs from ssv_queue_push"
        assert bool((bank[k:] == 7.0).all()), f"push {i}: rows >= K were touched"
        out[f"bank{i}"] = bank[:k].clone()
    return out


GPU = {"moco": _moco_gpu, "relic_kl": _relic_kl_gpu, "relic_whole": _relic_whole_gpu, "negdot": _pair_gpu, "mse": _pair_gpu, "cgrad": _cgrad_gpu,
       "barlow": _barlow_gpu, "dino": _dino_gpu, "center": _center_gpu, "ntxent": _ntxent_gpu, "ntxent_wide": _ntxent_gpu, "l2norm": _l2_gpu, "wn": _wn_gpu,
       "ce": _ce_gpu, "sgdn": _sgd_gpu, "sgd": _sgd_gpu, "adamw": _adamw_gpu, "elt": _elt_gpu, "queue": _queue_gpu}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_kernel_against_fp64(dev, case):
    from ssv_amd import ops
    fam, _, both, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    fails = []
    for arith in (("f32", "bf16x3") if both else ("f32",)):
        what = f"{case.id} [{arith}]"
        ctx = Ctx(dev)
        with ops.arithmetic(arith):
            got = GPU[case.kind](case, inp, ctx)
            torch.cuda.synchronize()
        assert set(got) == set(r64), what
        rec = REPORT.setdefault(what, {"family": fam})
        for name, ref64 in r64.items():
            g = got[name].detach().reshape(ref64.shape).cpu()
            assert torch.isfinite(g).all(), f"{what} {name}: non-finite values"
            (eg, mg), (er, mr) = _err(g, ref64), _err(r32[name], ref64)
            rec[name] = {"e_got": eg, "e_ref32": er, "m_got": mg, "m_ref32": mr}
            print(f"{what} {name}: e {eg:.3e} (ref32 {er:.3e}) m {mg:.3e} (ref32 {mr:.3e})")
            if not (eg <= FACTOR[fam] * er + FLOOR[fam] and mg <= FACTOR[fam] * mr + FLOOR[fam]):
                fails.append(f"{what} {name}: e {eg:.3e} vs ref32 {er:.3e}, m {mg:.3e} vs ref32 {mr:.3e} (FACTOR {FACTOR[fam]:g}, FLOOR {FLOOR[fam]:.2e})")
        ctx.verify(what)
    assert not fails, "\n".join(fails)
