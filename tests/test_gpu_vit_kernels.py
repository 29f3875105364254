"""Every kernel of the ViT / DINO encoder path that is not a GEMM (csrc/vit.hip: attention forward in two arithmetics, the three backward forms, LayerNorm,
GELU, token assembly; multicrop_k of csrc/augment.hip) against an fp64 evaluation of the same operation on the same fp32 inputs.

Each case of CASES names the entry points it reaches - all of them straight through the C ABI (_lib.call), so strides, guards and workspaces are the
test's own -, the branch labels it targets and a shape.  The inputs are drawn on the CPU from a generator seeded by the case id, so the GPU-free tests
below see exactly what the GPU tests upload.  Every run is held to:

  (a) for every tensor a case produces, with ref64 = plain torch in float64 on the CPU of the written-out operation, ref32 = the SAME lines in float32 on
      the CPU, e(x) = ||x - ref64||_2 / ||ref64||_2 and m(x) = max|x - ref64| / max|ref64|:
          e(got) <= FACTOR[family] * e(ref32) + FLOOR     and the same for m.
      e(ref32) comes from the reference, never from the library.  scale and eps enter both references as the fp32 value the ABI receives.
      Families: attention-forward (o, lse; both arithmetics, the worst ratio of each recorded separately), attention-backward (delta, dq, dk, dv),
      layernorm (y, mean, invstd, dx), elementwise (GELU, the bicubic resize), reduction (dcls / dpos, dgamma / dbeta); the token matrix is `exact`:
      bit-identical to the host restatement (oracle.vit.unfold_patches + concatenation);
  (b) a condition on the inputs: ref64 is finite and not identically zero, ref32 is within 1e-3 of it (e and m) - test_reference_is_well_conditioned;
  (c) every output is a 16-byte aligned view into a NaN-prefilled buffer with 1024 floats of guard behind it: no element the operation defines stays
      NaN, the guard and the padding columns (between heads * 64 and ldo / ldg, between the q, k and v blocks) are untouched, every input - its NaN
      padding columns included - is bit-identical afterwards;
  (d) the bitwise identities the sources state: ssv_attention_fwd == ssv_attention_fwd_arith(F32_MFMA); dense operands == strided slices of one
      matrix; a second call == the first; ssv_layernorm_bwd in place (dx_addend == dx, what ops.layernorm_bwd does) == a separate dx buffer; accumulate
      on a zero prior == overwrite; LayerNorm without addend gives the mean / invstd bits of the call with one; ssv_vit_embed_fwd through the vector
      kernel == through the scalar kernel (forced by a token pointer offset by 4 bytes).

The backward's operation is defined on its actual inputs (q, k, v, o, dout, lse, all fp32).  Both references evaluate
    P = exp(scale QK^T - lse), delta = rowsum(o * dout), dS = P * (dout V^T - delta), dQ = scale dS K, dK = scale dS^T Q, dV = P^T dout;
in the isolated cases (kind abwd) o and lse are ref64 of the forward rounded to fp32, so an error of the forward kernel can neither mask nor fake one of the
backward.  The composition cases (kind acomp: one per backward form at inputs x 1 and x 3) feed the library's own forward outputs, once from each
arithmetic, into the backward and compare with autograd of softmax(QK^T scale) V in fp64 (ref32: the same autograd in fp32).  At T = 1 (P = 1, o = v) dS is
the difference of two roundings of one sum: dq and dk have no conditioned reference there and are bounded by scale * 128 * 2^-24 * sum|dout v| * |k| (|q|).

multicrop_k's references are the kernel comment's formula written out: source index s (dst + 0.5) - 0.5 with s = h / Ho, A = -0.75, taps clamped to the
box.  The coordinate arithmetic is fp32 in both references so the taps agree; s (dst + 0.5) - 0.5 is rounded once, as the fused multiply-add the device
compiler contracts the expression into rounds it (separately rounded products move a coordinate of 30 by 2e-6, which is an input perturbation, not an
error of the interpolation).  Weights and sums are evaluated in the reference's own precision.

FACTOR: the worst max(0, e(got) - FLOOR) / e(ref32) (and the same for m) measured per family on an MI355X (profiles/vit_kernels_report.json, written by
this file under SSV_VIT_REPORT=<path>), rounded up to the next power of two and never above 8.  FLOOR = 2 * 2^-24.

The launch selection of vit.hip is restated below (attn_fwd_plan, attn_bwd_plan, ln_plan, embed_vector_route); test_restated_plan_is_the_source's pins the
thresholds those functions restate to the source text, test_case_shapes_have_the_property_their_label_claims holds every case to the property its
label names, so a retuned threshold fails here instead of silently hollowing the table out.

Branch labels (label, entry point, what the case reaches) - test_case_table_covers_every_documented_branch keeps CASES honest:

  fwd.nw2              ssv_attention_fwd_arith       T <= 64: two waves per workgroup (attn_fwd_k<2> and attn_fwd_sp_k<2>; every forward case runs both arithmetics)
  fwd.nw4              ssv_attention_fwd_arith       T > 64: four waves
  fwd.wave_idle        ssv_attention_fwd_arith       the workgroup's trailing waves own no query (T 1, 5, 16, 17, 31, 32; T 129: three of the second workgroup)
  fwd.wave_full        ssv_attention_fwd_arith       every wave of every workgroup owns queries
  fwd.slab_skip        ssv_attention_fwd_arith       the last key tile holds at most 16 keys: attn_fwd_sp_k skips its second 16-key slab
  fwd.slab_both        ssv_attention_fwd_arith       the last key tile holds more than 16 keys
  fwd.full_tile        ssv_attention_fwd_arith       T a multiple of 32: no key is masked
  fwd.wg2              ssv_attention_fwd_arith       more than one workgroup per (image, head)
  fwd.fused_ld         ssv_attention_fwd_arith       q, k, v column blocks of one matrix, ld = 3 hid, ldo = hid; the dense call gives the same bits
  fwd.dense_ld         ssv_attention_fwd_arith       ld = ldo = hid
  fwd.padded_ld        ssv_attention_fwd_arith       ld = hid + 4, ldo = hid + 8, padding columns NaN
  fwd.scale3           ssv_attention_fwd_arith       q and k x 3
  fwd.scale6           ssv_attention_fwd_arith       q and k x 6: logits past 100
  fwd.plant_first      ssv_attention_fwd_arith       key row 0 x 8: the maximum arrives in the first key tile
  fwd.plant_last       ssv_attention_fwd_arith       key row T - 1 x 8: the maximum arrives in the last key tile
  fwd.uniform          ssv_attention_fwd_arith       q = 0: P uniform, lse = log T
  fwd.dup_key          ssv_attention_fwd_arith       key row T - 1 a copy of key row 0
  bwd.fused2           ssv_attention_bwd             attn_bwd_fused_k<2>: T <= 64
  bwd.small_next       ssv_attention_bwd             32 < T <= 40: the second query tile staged with the first, one float4 per thread
  bwd.fused4           ssv_attention_bwd             attn_bwd_fused_k<4>: 64 < T <= 128
  bwd.fused8           ssv_attention_bwd             attn_bwd_fused_k<8>: 128 < T <= 256
  bwd.two_pass         ssv_attention_bwd             attn_bwd_dq_k<4> + attn_bwd_dkv_k<4>: T > 256
  bwd.g_fused          ssv_attention_bwd             dq, dk, dv column blocks of one matrix, ldg = 3 hid
  bwd.g_dense          ssv_attention_bwd             ldg = hid
  bwd.g_padded         ssv_attention_bwd             one gradient matrix of 3 hid + 12 columns: ldg is neither ld nor hid, NaN columns between the blocks
  bwd.ldo_padded       ssv_attention_bwd             o and dout with ldo = hid + 8
  bwd.scale3           ssv_attention_bwd             q and k x 3
  bwd.scale6           ssv_attention_bwd             q and k x 6
  bwd.plant_first      ssv_attention_bwd             key row 0 x 8
  bwd.plant_last       ssv_attention_bwd             key row T - 1 x 8
  comp.fused2          ssv_attention_bwd             the library's forward (each arithmetic) into attn_bwd_fused_k<2>, against fp64 autograd
  comp.fused4          ssv_attention_bwd             ... into attn_bwd_fused_k<4>
  comp.fused8          ssv_attention_bwd             ... into attn_bwd_fused_k<8>
  comp.two_pass        ssv_attention_bwd             ... into the two-pass form
  refuse.dh32          ssv_attention_fwd_arith       head size 32
  refuse.ld_mod4       ssv_attention_fwd_arith       ld % 4 != 0
  refuse.ld_short      ssv_attention_bwd             ld < heads * 64
  refuse.misaligned    ssv_attention_fwd             a pointer offset by 4 bytes
  refuse.arithmetic    ssv_attention_fwd_arith       an arithmetic nobody defined
  refuse.ln_c6         ssv_layernorm_fwd             C = 6
  refuse.ln_c2052      ssv_layernorm_bwd             C = 2052
  refuse.ln_ws         ssv_layernorm_bwd             a workspace one byte short
  refuse.gelu_n6       ssv_gelu_fwd                  n = 6
  refuse.embed_ragged  ssv_vit_embed_fwd             H % patch != 0
  ln.nit2              ssv_layernorm_fwd             C <= 512
  ln.nit4              ssv_layernorm_fwd             512 < C <= 1024
  ln.nit8              ssv_layernorm_fwd             1024 < C <= 2048
  ln.lane_ragged       ssv_layernorm_fwd             C is no multiple of 256: lanes past C hold zeros in the last trip
  ln.odd_rows          ssv_layernorm_fwd             M odd: the last wave's LNF_R = 2 pair has one live row
  ln.wg2               ssv_layernorm_fwd             M > 16: more than one forward workgroup
  ln.bwd_wave_ragged   ssv_layernorm_bwd             M % 8 != 0: a backward wave stops inside its 8 rows
  ln.bwd_block2        ssv_layernorm_bwd             M > 32: more than one backward block
  ln.addend            ssv_layernorm_fwd             addend / dx_addend given (and the in-place call)
  ln.acc               ssv_layernorm_bwd             accumulate 1 on a seeded prior (every other case: 0 on NaN-prefilled dgamma / dbeta)
  ln.offset            ssv_layernorm_fwd             row mean / std = 1000: the two-pass variance
  ln.const_row         ssv_layernorm_fwd             a constant row: variance 0, invstd = 1 / sqrt(eps)
  fin.per1             ssv_layernorm_bwd             at most 32 partial blocks: one per group of ln_bwd_finalize_k (nblocks 31: the last group empty)
  fin.per2             ssv_layernorm_bwd             nblocks 33: per = 2, groups past 17 empty
  fin.tail             ssv_layernorm_bwd             nblocks 161: per = 6, one unrolled trip and a tail of 2
  gelu.small           ssv_gelu_fwd                  n = 4, 1020, 1024, 1028: below, at and past one workgroup
  gelu.large           ssv_gelu_bwd                  n / 4 > 2^20
  embed.vector         ssv_vit_embed_fwd             vit_embed_fwd4_k; the scalar kernel (token pointer + 4 bytes) gives the same bits
  embed.nonsquare      ssv_vit_embed_fwd             H != W: pw = W / patch
  embed.p32            ssv_vit_embed_fwd             patch 32: P3 / 4 = 768 > 256 threads, F > 1024: the second trip of both loops of vit_embed_fwd4_k
  embed.f1024          ssv_vit_embed_fwd             F > 1024 through E = 1024
  embed.scalar_patch   ssv_vit_embed_fwd             patch % 4 != 0 with E % 4 == 0 (patch 6), and patch 40 > 32
  embed.scalar_e       ssv_vit_embed_fwd             E % 4 != 0
  embed.e0             ssv_vit_embed_fwd             E = 0
  embedb.chains        ssv_vit_embed_bwd             B around the four interleaved chains: 1, 7, 8, 9, 24, 25, 32, 33, 57
  embedb.cols32        ssv_vit_embed_bwd             P3 + T E a multiple of 32 (otherwise: a ragged last workgroup)
  embedb.e0            ssv_vit_embed_bwd             E = 0
  embedb.acc           ssv_vit_embed_bwd             accumulate 1 on a prior; rows of dpos past T stay untouched in every case
  crop.boxes           ssv_multicrop                 24 x 40 source, B 3, 5 crops, every (b, crop) its own box: full image, four corners, h or w of 1, 2, 3, 1 x 1
  crop.oracle          ssv_multicrop                 also against oracle.vit.multicrop_resize (torch's bicubic interpolate)

Measured on an MI355X (profiles/vit_kernels_report.json): see FACTOR below and DESIGN.md section 2.
"""
import json
import math
import os
import re
import zlib

import pytest
import torch

U = 2.0 ** -24
GUARD = 1024                                                             # floats of NaN behind every output
WS_GUARD = 4096                                                          # ... and behind a workspace
LN_EPS = 1e-5
DH = 64
ARITH = {"f32": 0, "bf16x3": 6}                                          # SSV_ARITH_F32_MFMA, SSV_ARITH_BF16X3 (include/ssv_hip.h)
# one FACTOR per family, set by the rule of the docstring from the MI355X run committed as profiles/vit_kernels_report.json.  Measured worst ratios:
# attention-forward 2.50 (o of the fp32 forward at T 65, three heads; per arithmetic: fp32 2.50, bf16x3 1.42), attention-backward 6.16 (dv of the T 37
# composition at inputs x 3 behind the bf16x3 forward; the isolated backward stays at 2.51), layernorm 0.78 (y at mean / std = 1000), elementwise 0.59
# (the 7 x 13 bicubic resize), reduction 0.80 (dgamma at C 4, M 33).
FACTOR = {"attention-forward": 4.0, "attention-backward": 8.0, "layernorm": 1.0, "elementwise": 1.0, "reduction": 1.0}
FLOOR = 2 * U                                                            # the final rounding of an fp32 result, twice where a prior is added
COND = 1e-3                                                              # (b): ref32 further than this from ref64 measures nothing
REPORT = {}                                                              # case id -> tensor -> figures (SSV_VIT_REPORT)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "self-supervised-vision_amd", "csrc")

FAMILY = {}
for _fam, _names in (("attention-forward", "o_f32 lse_f32 o_bf16x3 lse_bf16x3"),
                     ("attention-backward", "delta dq dk dv dq_f32 dk_f32 dv_f32 dq_bf16x3 dk_bf16x3 dv_bf16x3"),
                     ("layernorm", "y mean invstd dx"),
                     ("elementwise", "gelu_y gelu_dx crop"),
                     ("reduction", "dcls dpos dgamma dbeta"),
                     ("exact", "tok")):
    FAMILY.update({n: _fam for n in _names.split()})


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


def cdiv(a, b):
    return -(-a // b)


# ====================================================================================================================== the launch selection, restated
def attn_fwd_plan(t):
    """ssv_attention_fwd_arith, both arithmetics: waves per workgroup, workgroups per (image, head), waves without a query, keys of the last key tile"""
    nw = 2 if t <= 64 else 4
    wgs = cdiv(t, 32 * nw)
    return {"NW": nw, "wgs": wgs, "idle": wgs * nw - cdiv(t, 32), "last_keys": t - (cdiv(t, 32) - 1) * 32}


def attn_bwd_plan(t):
    """ssv_attention_bwd: the one-pass form up to 256 tokens (2, 4 or 8 waves), else dQ and dK / dV in two passes of four-wave workgroups"""
    if t > 256:
        return {"form": "two_pass", "NW": 4, "small_next": False}
    nw = 2 if t <= 64 else 4 if t <= 128 else 8
    return {"form": "fused", "NW": nw, "small_next": nw == 2 and 32 < t <= 40}


def ln_plan(m, c):
    """LayerNorm: 256-column trips per lane, forward workgroups of 4 waves x LNF_R 2 x LNF_TRIPS 2 rows, backward blocks of LN_ROWS 32 (8 per wave), the finalize's grouping"""
    nblocks = cdiv(m, 32)
    return {"NIT": 2 if c <= 512 else 4 if c <= 1024 else 8, "fwd_wgs": cdiv(m, 16), "nblocks": nblocks, "per": cdiv(nblocks, 32), "ws_bytes": nblocks * 2 * c * 4}


def embed_vector_route(patch, e, aligned=True):
    """ssv_vit_embed_fwd launches vit_embed_fwd4_k"""
    return patch % 4 == 0 and patch <= 32 and e % 4 == 0 and aligned


SOURCE_PINS = (                                                          # what the functions above restate, as vit.hip spells it
    r"if \(T <= 64\) hipLaunchKernelGGL\(attn_fwd_sp_k<2>, dim3\(cdiv\(T, 64\), heads, B\)",
    r"else hipLaunchKernelGGL\(attn_fwd_sp_k<4>, dim3\(cdiv\(T, 128\), heads, B\)",
    r"else if \(T <= 64\) hipLaunchKernelGGL\(attn_fwd_k<2>, dim3\(cdiv\(T, 64\), heads, B\)",
    r"else hipLaunchKernelGGL\(attn_fwd_k<4>, dim3\(cdiv\(T, 128\), heads, B\)",
    r"if \(k0 \+ 16 \* sp >= T\) continue;",
    r"if \(T <= 256\) \{",
    r"if \(T <= 64\) hipLaunchKernelGGL\(attn_bwd_fused_k<2>",
    r"else if \(T <= 128\) hipLaunchKernelGGL\(attn_bwd_fused_k<4>",
    r"else hipLaunchKernelGGL\(attn_bwd_fused_k<8>",
    r"hipLaunchKernelGGL\(attn_bwd_dq_k<4>, grid, dim3\(256\)",
    r"hipLaunchKernelGGL\(attn_bwd_dkv_k<4>, grid, dim3\(256\)",
    r"const dim3 grid\(cdiv\(T, 128\), heads, B\);\s*// T > 256: two passes of four-wave workgroups\n  hipLaunchKernelGGL\(attn_bwd_dq_k<4>",
    r"const bool small_next = NW == 2 && T > 32 && T <= 40;",
    r"constexpr int LNF_R = 2;",
    r"constexpr int LNF_TRIPS = 2;",
    r"constexpr int LN_ROWS = 32;",
    r"if \(C <= 512\) hipLaunchKernelGGL\(ln_fwd_k<2>",
    r"else if \(C <= 1024\) hipLaunchKernelGGL\(ln_fwd_k<4>",
    r"if \(C <= 512\) hipLaunchKernelGGL\(ln_bwd_k<2>",
    r"else if \(C <= 1024\) hipLaunchKernelGGL\(ln_bwd_k<4>",
    r"const int per = \(nblocks \+ 31\) / 32;",
    r"for \(; b \+ 3 < b1; b \+= 4\)",
    r"constexpr int EMB_MAXP = 32;",
    r"if \(patch % 4 == 0 && patch <= EMB_MAXP && E % 4 == 0 && \(\(\(uintptr_t\)img_nhwc \| \(uintptr_t\)cls \| \(uintptr_t\)pos \| \(uintptr_t\)tokens\) & 15\) == 0",
    r"for \(int f = 4 \* threadIdx.x; f < F; f \+= 1024\)",
    r"for \(; bb \+ 24 < B; bb \+= 32\)",
    r"dim3\(cdiv\(P3 \+ T \* E, 32\)\)",
)


# ====================================================================================================================== inputs and references
# Every kind has inputs(case) -> {name: CPU tensor} and ref(case, inputs, dtype) -> {name: tensor}: plain torch, run in float64 and in float32.
# Nothing here touches the library or the GPU.
def _split(x, b, t, h):
    return x.view(b, t, h, DH).transpose(1, 2)                           # [B*T, heads*64] -> [B, heads, T, 64]


def _merge(x):
    b, h, t, _ = x.shape
    return x.transpose(1, 2).reshape(b * t, h * DH)


def _attn_fwd_lines(q, k, v, scale, b, t, h):
    s = (_split(q, b, t, h) @ _split(k, b, t, h).transpose(-1, -2)) * scale
    mx = s.amax(-1, keepdim=True)
    p = (s - mx).exp()
    l = p.sum(-1, keepdim=True)
    return _merge((p / l) @ _split(v, b, t, h)), (mx + l.log()).squeeze(-1)


def _attn_bwd_lines(q, k, v, o, dout, lse, scale, b, t, h):
    qh, kh, vh, oh, gh = (_split(x, b, t, h) for x in (q, k, v, o, dout))
    p = ((qh @ kh.transpose(-1, -2)) * scale - lse[..., None]).exp()
    delta = (oh * gh).sum(-1)
    ds = p * (gh @ vh.transpose(-1, -2) - delta[..., None])
    return delta, _merge(scale * (ds @ kh)), _merge(scale * (ds.transpose(-1, -2) @ qh)), _merge(p.transpose(-1, -2) @ gh)


def _attn_in(c):
    g = c.gen()
    b, t, h = c["B"], c["T"], c["heads"]
    m, hid = b * t, h * DH
    q, k, v, dout = (_rn(g, m, hid) for _ in range(4))
    mult = float(c["mult"] or 1)
    q, k = q * mult, k * mult
    kk = k.view(b, t, hid)
    mode = c["mode"]
    if mode == "plant0":
        kk[:, 0] *= 8.0
    if mode == "plantL":
        kk[:, t - 1] *= 8.0
    if mode == "zero_q":
        q.zero_()
    if mode == "dup":
        kk[:, t - 1] = kk[:, 0]
    inp = {"q": q, "k": k, "v": v, "dout": dout}
    o64, lse64 = _attn_fwd_lines(q.double(), k.double(), v.double(), _s(DH ** -0.5), b, t, h)
    inp["o_in"], inp["lse_in"] = o64.float(), lse64.float()             # the backward's o and lse are data: the fp64 forward's, rounded to fp32
    return inp


def _afwd_ref(c, inp, dt):
    q, k, v = _t(inp, dt, "q", "k", "v")
    o, lse = _attn_fwd_lines(q, k, v, _s(DH ** -0.5), c["B"], c["T"], c["heads"])
    return {"o_f32": o, "lse_f32": lse, "o_bf16x3": o, "lse_bf16x3": lse}


def _abwd_ref(c, inp, dt):
    q, k, v, o, dout, lse = _t(inp, dt, "q", "k", "v", "o_in", "dout", "lse_in")
    delta, dq, dk, dv = _attn_bwd_lines(q, k, v, o, dout, lse, _s(DH ** -0.5), c["B"], c["T"], c["heads"])
    if c["T"] == 1:                                                      # P == 1 and o == v: dS is the difference of two roundings of one sum, dq and dk are noise
        return {"delta": delta, "dv": dv}                                # (_abwd_gpu bounds them instead)
    return {"delta": delta, "dq": dq, "dk": dk, "dv": dv}


def _acomp_ref(c, inp, dt):
    b, t, h = c["B"], c["T"], c["heads"]
    q, k, v, dout = _t(inp, dt, "q", "k", "v", "dout")
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    s = (_split(q, b, t, h) @ _split(k, b, t, h).transpose(-1, -2)) * _s(DH ** -0.5)
    _merge(torch.softmax(s, -1) @ _split(v, b, t, h)).backward(dout)
    out = {}
    for a in ARITH:
        out.update({f"dq_{a}": q.grad, f"dk_{a}": k.grad, f"dv_{a}": v.grad})
    return out


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------------------
def _ln_in(c):
    g = c.gen()
    m, ch = c["M"], c["C"]
    mu, sd = float(c["mean"] or 0.0), float(c["std"] or 1.0)
    x = _rn(g, m, ch, scale=sd) + mu
    if c["const_row"]:
        x[0] = 0.5                                                       # every partial sum of the row is exact: mean == 0.5, x - mean == 0
    inp = {"x": x, "gamma": torch.rand(ch, generator=g) + 0.5, "beta": _rn(g, ch, scale=0.3), "addend": _rn(g, m, ch), "dy": _rn(g, m, ch),
           "dx_addend": _rn(g, m, ch), "dg0": _rn(g, ch), "db0": _rn(g, ch)}
    x64 = x.double()
    mean = x64.mean(1)
    inp["mean_in"] = mean.float()                                        # the backward's statistics are data: the fp64 ones, rounded to fp32
    inp["invstd_in"] = (1.0 / (((x64 - mean[:, None]) ** 2).mean(1) + _s(LN_EPS)).sqrt()).float()
    return inp


def _ln_ref(c, inp, dt):
    x, gamma, beta, dy, mean_in, invstd_in, dg0, db0 = _t(inp, dt, "x", "gamma", "beta", "dy", "mean_in", "invstd_in", "dg0", "db0")
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    invstd = 1.0 / (var + _s(LN_EPS)).sqrt()
    y = (x - mean[:, None]) * invstd[:, None] * gamma + beta
    xh = (x - mean_in[:, None]) * invstd_in[:, None]
    gv = dy * gamma
    dx = invstd_in[:, None] * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    if c["addend"]:
        y, dx = y + inp["addend"].to(dt), dx + inp["dx_addend"].to(dt)
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    if c["acc"]:
        dgamma, dbeta = dgamma + dg0, dbeta + db0
    return {"y": y, "mean": mean, "invstd": invstd, "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


# ---- GELU (erf form) --------------------------------------------------------------------------------------------------------------------------------
def _gelu_in(c):
    g = c.gen()
    return {"x": _rn(g, c["n"], scale=3.0), "dy": _rn(g, c["n"])}


def _gelu_ref(c, inp, dt):
    x, dy = _t(inp, dt, "x", "dy")
    cdf = 0.5 * (1.0 + torch.erf(x * (0.5 ** 0.5)))
    pdf = torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))
    return {"gelu_y": x * cdf, "gelu_dx": dy * (cdf + x * pdf)}


# ---- token assembly ---------------------------------------------------------------------------------------------------------------------------------
def _embed_in(c):
    g = c.gen()
    b, h, w, patch, e = c["B"], c["H"], c["W"], c["patch"], c["E"]
    t = (h // patch) * (w // patch) + 1
    return {"img": _rn(g, b, 3, h, w), "cls": _rn(g, 1, 3 * patch * patch), "pos": _rn(g, t + 3, max(e, 1))[:, :e].contiguous()}


def _embed_ref(c, inp, dt):
    from oracle import vit as ovit
    b, patch = c["B"], c["patch"]
    x = ovit.unfold_patches(inp["img"], patch)
    n = x.shape[1]
    tok = torch.cat([torch.cat([inp["cls"].expand(b, 1, -1), x], 1), inp["pos"][:n + 1].expand(b, -1, -1)], -1)
    return {"tok": tok.reshape(b * (n + 1), -1).to(dt)}


def _embedb_in(c):
    g = c.gen()
    b, t, p3, e = c["B"], c["T"], c["P3"], c["E"]
    return {"dtok": _rn(g, b, t, p3 + e), "dcls0": _rn(g, p3), "dpos0": _rn(g, t + 2, max(e, 1))[:, :e].contiguous()}


def _embedb_ref(c, inp, dt):
    dtok, dcls0, dpos0 = _t(inp, dt, "dtok", "dcls0", "dpos0")
    p3, t = c["P3"], c["T"]
    dcls, dpos = dtok[:, 0, :p3].sum(0), dtok[:, :, p3:].sum(0)
    if c["acc"]:
        dcls, dpos = dcls + dcls0, dpos + dpos0[:t]
    out = {"dcls": dcls}
    if c["E"]:
        out["dpos"] = dpos
    return out


# ---- multi-crop: crop + bicubic resize ----------------------------------------------------------------------------------------------------------------
CROP_SRC = (24, 40)
CROP_BOXES = (                                                           # (top, left, h, w): B 3 x 5 crops, every one its own
    (0, 0, 24, 40), (0, 0, 5, 7), (0, 33, 5, 7), (19, 0, 5, 7), (19, 33, 5, 7),
    (3, 4, 1, 9), (10, 2, 2, 11), (20, 25, 3, 14), (2, 5, 8, 1), (7, 38, 16, 2),
    (0, 17, 24, 3), (23, 39, 1, 1), (4, 6, 13, 20), (1, 17, 22, 9), (11, 0, 2, 2),
)


def _crop_in(c):
    g = c.gen()
    return {"views": _rn(g, 3, CROP_SRC[0], CROP_SRC[1], 3), "boxes": torch.tensor(CROP_BOXES, dtype=torch.int32).view(3, 5, 4)}


def _cubic(t):
    a = -0.75
    outer = lambda x: ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    inner = lambda x: ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    return torch.stack((outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)), 1)


def _crop_axis(n_src, n_dst, dt):
    """per destination index: the four clamped taps (relative to the box) and their weights.  Coordinates in fp32, s (dst + 0.5) - 0.5 rounded once"""
    s = torch.tensor(float(n_src), dtype=torch.float32) / torch.tensor(float(n_dst), dtype=torch.float32)
    r = (s.double() * (torch.arange(n_dst, dtype=torch.float32) + 0.5).double() - 0.5).float()
    f = r.floor()
    taps = (f.long()[:, None] - 1 + torch.arange(4)).clamp(0, n_src - 1)
    return taps, _cubic((r - f).to(dt))


def _crop_ref(c, inp, dt):
    ho, wo = c["size"]
    views = inp["views"].to(dt)
    out = torch.empty(3, 5, ho, wo, 3, dtype=dt)
    for b in range(3):
        for j in range(5):
            top, left, h, w = (int(x) for x in inp["boxes"][b, j])
            (iy, wy), (ix, wx) = _crop_axis(h, ho, dt), _crop_axis(w, wo, dt)
            taps = views[b][top + iy][:, :, left + ix]                  # [Ho, 4, Wo, 4, 3]
            out[b, j] = torch.einsum("yaxcz,ya,xc->yxz", taps, wy, wx)
    return {"crop": out}


def _no_ref(c, inp, dt):
    return {}


# ====================================================================================================================== the case table
KINDS = {
    # kind: (entry points reached, inputs, reference)
    "afwd": ("ssv_attention_fwd ssv_attention_fwd_arith", _attn_in, _afwd_ref),
    "abwd": ("ssv_attention_bwd", _attn_in, _abwd_ref),
    "acomp": ("ssv_attention_fwd_arith ssv_attention_bwd", _attn_in, _acomp_ref),
    "ln": ("ssv_layernorm_fwd ssv_layernorm_bwd", _ln_in, _ln_ref),
    "gelu": ("ssv_gelu_fwd ssv_gelu_bwd", _gelu_in, _gelu_ref),
    "embed": ("ssv_vit_embed_fwd", _embed_in, _embed_ref),
    "embedb": ("ssv_vit_embed_bwd", _embedb_in, _embedb_ref),
    "crop": ("ssv_multicrop", _crop_in, _crop_ref),
    "refuse": ("ssv_attention_fwd ssv_attention_fwd_arith ssv_attention_bwd ssv_layernorm_fwd ssv_layernorm_bwd ssv_gelu_fwd ssv_vit_embed_fwd", lambda c: {}, _no_ref),
}
ENTRY_POINTS = "ssv_attention_fwd ssv_attention_fwd_arith ssv_attention_bwd ssv_layernorm_fwd ssv_layernorm_bwd ssv_gelu_fwd ssv_gelu_bwd ssv_vit_embed_fwd " \
               "ssv_vit_embed_bwd ssv_multicrop"


def _fwd_labels(t, layout, mode, mult):
    p = attn_fwd_plan(t)
    out = ["fwd.nw2" if p["NW"] == 2 else "fwd.nw4", "fwd.wave_idle" if p["idle"] else "fwd.wave_full", "fwd.slab_skip" if p["last_keys"] <= 16 else "fwd.slab_both",
           f"fwd.{layout}_ld"]
    if t % 32 == 0:
        out.append("fwd.full_tile")
    if p["wgs"] > 1:
        out.append("fwd.wg2")
    if mult in (3, 6):
        out.append(f"fwd.scale{mult}")
    if mode:
        out.append({"plant0": "fwd.plant_first", "plantL": "fwd.plant_last", "zero_q": "fwd.uniform", "dup": "fwd.dup_key"}[mode])
    return " ".join(out)


def _afwd(t, b, heads, layout, mode=None, mult=1):
    p = {"B": b, "T": t, "heads": heads, "layout": layout}
    if mode:
        p["mode"] = mode
    if mult != 1:
        p["mult"] = mult
    return Case("afwd", _fwd_labels(t, layout, mode, mult), **p)


def _bwd_labels(t, ld, ldo, ldg, mode, mult):
    p = attn_bwd_plan(t)
    out = ["bwd.two_pass" if p["form"] == "two_pass" else f"bwd.fused{p['NW']}", f"bwd.g_{ldg}"]
    if p["small_next"]:
        out.append("bwd.small_next")
    if ldo == "padded":
        out.append("bwd.ldo_padded")
    if mult in (3, 6):
        out.append(f"bwd.scale{mult}")
    if mode:
        out.append({"plant0": "bwd.plant_first", "plantL": "bwd.plant_last"}[mode])
    return " ".join(out)


def _abwd(t, b, heads, ld, ldo, ldg, mode=None, mult=1):
    p = {"B": b, "T": t, "heads": heads, "layout": ld, "ldo": ldo, "ldg": ldg}
    if mode:
        p["mode"] = mode
    if mult != 1:
        p["mult"] = mult
    return Case("abwd", _bwd_labels(t, ld, ldo, ldg, mode, mult), **p)


def _acomp(t, mult):
    p = attn_bwd_plan(t)
    label = "comp.two_pass" if p["form"] == "two_pass" else f"comp.fused{p['NW']}"
    return Case("acomp", label, B=2 if t < 200 else 1, T=t, heads=2 if t < 200 else 1, mult=mult)


def _ln(m, c, addend=False, acc=False, **kw):
    p = ln_plan(m, c)
    out = [f"ln.nit{p['NIT']}"]
    if c % 256:
        out.append("ln.lane_ragged")
    if m % 2:
        out.append("ln.odd_rows")
    if p["fwd_wgs"] > 1:
        out.append("ln.wg2")
    if m % 8:
        out.append("ln.bwd_wave_ragged")
    if p["nblocks"] > 1:
        out.append("ln.bwd_block2")
    if addend:
        out.append("ln.addend")
    if acc:
        out.append("ln.acc")
    if kw.get("mean"):
        out.append("ln.offset")
    if kw.get("const_row"):
        out.append("ln.const_row")
    out.append("fin.per1" if p["per"] == 1 else "fin.per2" if p["per"] == 2 else "fin.tail")
    return Case("ln", " ".join(out), M=m, C=c, addend=addend, acc=acc, **kw)


def _embed(b, h, w, patch, e):
    out = []
    if embed_vector_route(patch, e):
        out.append("embed.vector")
    if h != w:
        out.append("embed.nonsquare")
    if patch == 32:
        out.append("embed.p32")
    if e >= 1024:
        out.append("embed.f1024")
    if patch % 4 or patch > 32:
        out.append("embed.scalar_patch")
    if e % 4:
        out.append("embed.scalar_e")
    if e == 0:
        out.append("embed.e0")
    return Case("embed", " ".join(out), B=b, H=h, W=w, patch=patch, E=e)


def _embedb(b, t, p3, e, acc):
    out = ["embedb.chains"]
    if (p3 + t * e) % 32 == 0:
        out.append("embedb.cols32")
    if e == 0:
        out.append("embedb.e0")
    if acc:
        out.append("embedb.acc")
    return Case("embedb", " ".join(out), B=b, T=t, P3=p3, E=e, acc=acc)


_L3 = ("fused", "dense", "padded")
FWD_T = (1, 5, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 161, 197, 256, 257, 300)
BWD_T = {"fused2": (1, 5, 31, 32, 33, 37, 40, 41, 48, 63, 64), "fused4": (65, 96, 97, 127, 128), "fused8": (129, 161, 197, 225, 256), "two_pass": (257, 289, 300, 385)}
LN_C = (4, 252, 256, 260, 384, 512, 516, 1024, 1028, 2044, 2048)
LN_M = (1, 2, 3, 15, 16, 17, 31, 32, 33, 65)
_LN_PAIRS = ((1, 33), (2, 17), (3, 65), (15, 32), (16, 31))

CASES = [
    # ---- attention forward: every T at inputs x 1, layouts / heads / B rotating; both arithmetics inside every case
    *[_afwd(t, (1, 3)[i % 2], (1, 2, 3, 6)[i % 4] if t <= 161 else (2, 1)[i % 2], _L3[i % 3]) for i, t in enumerate(FWD_T)],
    # ---- ... the input modes at one T per kernel shape (two waves; second workgroup with idle waves; the longest)
    *[_afwd(t, 1 if t > 200 else 2, 1 if t > 200 else 2, _L3[(i + j) % 3], mode, mult)
      for j, t in enumerate((33, 129, 300))
      for i, (mode, mult) in enumerate(((None, 3), (None, 6), ("plant0", 1), ("plantL", 1), ("zero_q", 1), ("dup", 1)))],
    _afwd(17, 3, 3, "padded", "plantL", 3),
    _afwd(64, 1, 6, "fused", None, 6),
    # ---- attention backward, isolated: every T of every form; input layout, ldo, gradient layout, scale and planted keys rotating
    *[_abwd(t, (1, 3, 2)[i % 3], (2, 1, 3)[i % 3] if t <= 128 else 1 + i % 2, _L3[i % 3], ("dense", "padded")[i % 2], ("fused", "dense", "padded")[(i + i // 3) % 3],
            (None, None, "plant0", None, "plantL")[i % 5], (1, 3, 1, 6, 1)[i % 5])
      for i, t in enumerate(t for form in BWD_T.values() for t in form)],
    # ---- ... small_next and its neighbours once more at the large scale, and the shipped shapes as they ship (fused qkv, fused gradient matrix)
    _abwd(37, 5, 6, "fused", "dense", "fused", None, 6),
    _abwd(40, 2, 2, "padded", "padded", "padded", "plantL", 3),
    _abwd(41, 2, 2, "padded", "padded", "padded", "plantL", 3),
    _abwd(33, 2, 3, "dense", "dense", "dense", "plant0", 3),
    _abwd(197, 2, 6, "fused", "dense", "fused", None, 3),
    _abwd(300, 1, 2, "fused", "padded", "padded", "plant0", 6),
    # ---- compositions: the library's own forward (each arithmetic) into each backward form
    *[_acomp(t, mult) for t in (37, 97, 197, 300) for mult in (1, 3)],
    # ---- LayerNorm: every M with C 384, every C with two M; addend and accumulate alternate
    *[_ln(m, 384, addend=bool(i % 2), acc=bool((i // 2) % 2)) for i, m in enumerate(LN_M)],
    *[_ln(m, c, addend=bool((i + j) % 2), acc=bool(j % 2)) for i, c in enumerate(c for c in LN_C if c != 384) for j, m in enumerate(_LN_PAIRS[i % 5])],
    _ln(8, 384, addend=True, acc=True),
    _ln(990, 384, addend=True, acc=False),
    _ln(1030, 64, addend=False, acc=True),
    _ln(5121, 8, addend=True, acc=True),
    _ln(33, 384, addend=True, acc=False, mean=30.0, std=0.03),
    _ln(17, 1028, addend=False, acc=True, mean=30.0, std=0.03),
    _ln(9, 384, addend=False, acc=False, const_row=True),
    # ---- GELU
    *[Case("gelu", "gelu.small", n=n) for n in (4, 1020, 1024, 1028)],
    Case("gelu", "gelu.large", n=4 * ((1 << 20) + 3)),
    # ---- token assembly forward: (B, H, W, patch, E)
    _embed(3, 8, 16, 4, 8),
    _embed(3, 16, 8, 4, 8),
    _embed(2, 32, 96, 16, 64),
    _embed(2, 64, 32, 32, 4),
    _embed(2, 40, 80, 40, 8),
    _embed(3, 12, 18, 6, 8),
    _embed(5, 8, 12, 4, 6),
    _embed(3, 8, 12, 4, 0),
    _embed(3, 12, 18, 6, 0),
    _embed(3, 8, 12, 4, 1024),
    # ---- token assembly backward: (B, T, P3, E)
    *[_embedb(b, (3, 5)[i % 2], 12, 4, bool(i % 2)) for i, b in enumerate((1, 7, 8, 9, 24, 25, 32, 33, 57))],
    _embedb(25, 2, 48, 0, False),
    _embedb(33, 2, 27, 0, True),
    _embedb(57, 6, 27, 5, False),
    # ---- multi-crop: output size
    Case("crop", "crop.boxes crop.oracle", size=(7, 13)),
    Case("crop", "crop.boxes", size=(32, 32)),
    Case("crop", "crop.boxes", size=(1, 1)),
    # ---- refusals
    *[Case("refuse", f"refuse.{w}", what=w) for w in ("dh32", "ld_mod4", "ld_short", "misaligned", "arithmetic", "ln_c6", "ln_c2052", "ln_ws", "gelu_n6", "embed_ragged")],
]


# ====================================================================================================================== GPU-free honesty tests
def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(\S+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def test_case_table_names_every_entry_point():
    """GPU-free: the entry points named by CASES are the ten of the ViT path, and vit.hip exports no launching entry point this file leaves out."""
    named = {e for c in CASES for e in KINDS[c.kind][0].split()}
    assert named == set(ENTRY_POINTS.split()), sorted(named ^ set(ENTRY_POINTS.split()))
    with open(os.path.join(CSRC, "vit.hip")) as f:
        have = set(re.findall(r'^extern "C" int (ssv_\w+)\(', f.read(), flags=re.M))
    assert have and have <= named, f"vit.hip exports {sorted(have - named)} without a case"
    with open(os.path.join(CSRC, "augment.hip")) as f:
        assert 'extern "C" int ssv_multicrop(' in f.read()


def test_restated_plan_is_the_source():
    """GPU-free: every threshold that attn_fwd_plan, attn_bwd_plan, ln_plan and embed_vector_route restate stands in vit.hip (with the attention pieces of
    attention_tile.h) as restated; the two-pass backward names only its four-wave kernels."""
    src = ""
    for name in ("vit.hip", "attention_tile.h"):
        with open(os.path.join(CSRC, name)) as f:
            src += f.read()
    for pin in SOURCE_PINS:
        assert re.search(pin, src), f"vit.hip no longer says {pin!r}: restate the plan in this file and re-derive the case table"
    assert "attn_bwd_dq_k<2>" not in src and "attn_bwd_dkv_k<2>" not in src, "the two-pass backward has a two-wave form again: attn_bwd_plan restates NW 4 only"
    assert set(re.findall(r"hipLaunchKernelGGL\(attn_bwd_d(?:q|kv)_k<(\d+)>", src)) == {"4"} and src.count("hipLaunchKernelGGL(attn_bwd_dq_k<") == 1
    assert src.count("hipLaunchKernelGGL(attn_bwd_dkv_k<") == 1
    assert src.count("hipLaunchKernelGGL(attn_bwd_fused_k<") == 3 and src.count("hipLaunchKernelGGL(ln_fwd_k<") == 3 and src.count("hipLaunchKernelGGL(ln_bwd_k<") == 3


def test_case_table_covers_every_documented_branch():
    """GPU-free: every branch label of the docstring has a case, every label of a case is documented, the documented entry point is one the case's
    kind reaches, ids are unique, every output name has a family, and the bounds respect their caps."""
    doc = documented_labels()
    assert len(doc) >= 70
    used = {b for c in CASES for b in c.labels}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    for label, entry in doc.items():
        assert any(label in c.labels and entry in KINDS[c.kind][0].split() for c in CASES), (label, entry)
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(FAMILY.values()) - {"exact"} == set(FACTOR) and len(FACTOR) == 5
    assert all(1.0 <= f <= 8.0 and math.log2(f).is_integer() for f in FACTOR.values())
    assert FLOOR == 2 * U


def _fin(c):
    return ln_plan(c["M"], c["C"])


PROPERTY = {
    "fwd.nw2": lambda c: c["T"] <= 64 and attn_fwd_plan(c["T"])["NW"] == 2,
    "fwd.nw4": lambda c: c["T"] > 64 and attn_fwd_plan(c["T"])["NW"] == 4,
    "fwd.wave_idle": lambda c: attn_fwd_plan(c["T"])["idle"] > 0,
    "fwd.wave_full": lambda c: attn_fwd_plan(c["T"])["idle"] == 0,
    "fwd.slab_skip": lambda c: 1 <= c["T"] - (cdiv(c["T"], 32) - 1) * 32 <= 16,
    "fwd.slab_both": lambda c: c["T"] - (cdiv(c["T"], 32) - 1) * 32 > 16,
    "fwd.full_tile": lambda c: c["T"] % 32 == 0,
    "fwd.wg2": lambda c: cdiv(c["T"], 32 * attn_fwd_plan(c["T"])["NW"]) >= 2,
    "fwd.scale3": lambda c: c["mult"] == 3, "fwd.scale6": lambda c: c["mult"] == 6,
    "fwd.plant_first": lambda c: c["mode"] == "plant0" and c["T"] > 32, "fwd.plant_last": lambda c: c["mode"] == "plantL",
    "fwd.uniform": lambda c: c["mode"] == "zero_q", "fwd.dup_key": lambda c: c["mode"] == "dup" and c["T"] >= 2,
    "bwd.fused2": lambda c: c["T"] <= 64 and attn_bwd_plan(c["T"]) == {"form": "fused", "NW": 2, "small_next": 32 < c["T"] <= 40},
    "bwd.small_next": lambda c: 32 < c["T"] <= 40 and attn_bwd_plan(c["T"])["small_next"],
    "bwd.fused4": lambda c: 64 < c["T"] <= 128 and attn_bwd_plan(c["T"])["NW"] == 4 and attn_bwd_plan(c["T"])["form"] == "fused",
    "bwd.fused8": lambda c: 128 < c["T"] <= 256 and attn_bwd_plan(c["T"])["NW"] == 8,
    "bwd.two_pass": lambda c: c["T"] > 256 and attn_bwd_plan(c["T"])["form"] == "two_pass",
    "bwd.g_fused": lambda c: c["ldg"] == "fused", "bwd.g_dense": lambda c: c["ldg"] == "dense", "bwd.g_padded": lambda c: c["ldg"] == "padded",
    "bwd.ldo_padded": lambda c: c["ldo"] == "padded",
    "bwd.scale3": lambda c: c["mult"] == 3, "bwd.scale6": lambda c: c["mult"] == 6,
    "bwd.plant_first": lambda c: c["mode"] == "plant0", "bwd.plant_last": lambda c: c["mode"] == "plantL",
    "comp.fused2": lambda c: attn_bwd_plan(c["T"])["NW"] == 2 and c["T"] <= 64, "comp.fused4": lambda c: 64 < c["T"] <= 128,
    "comp.fused8": lambda c: 128 < c["T"] <= 256, "comp.two_pass": lambda c: c["T"] > 256,
    "ln.nit2": lambda c: c["C"] <= 512 and _fin(c)["NIT"] == 2, "ln.nit4": lambda c: 512 < c["C"] <= 1024 and _fin(c)["NIT"] == 4,
    "ln.nit8": lambda c: 1024 < c["C"] <= 2048 and _fin(c)["NIT"] == 8,
    "ln.lane_ragged": lambda c: c["C"] % 256 != 0,
    "ln.odd_rows": lambda c: c["M"] % 2 == 1,
    "ln.wg2": lambda c: _fin(c)["fwd_wgs"] >= 2,
    "ln.bwd_wave_ragged": lambda c: c["M"] % 8 != 0,
    "ln.bwd_block2": lambda c: _fin(c)["nblocks"] >= 2,
    "ln.addend": lambda c: c["addend"], "ln.acc": lambda c: c["acc"],
    "ln.offset": lambda c: c["mean"] / c["std"] >= 999,
    "ln.const_row": lambda c: c["const_row"] and not c["mean"],
    "fin.per1": lambda c: _fin(c)["per"] == 1,
    "fin.per2": lambda c: _fin(c)["per"] == 2 and _fin(c)["nblocks"] == 33,
    "fin.tail": lambda c: _fin(c)["nblocks"] >= 161 and _fin(c)["per"] > 4 and _fin(c)["per"] % 4 != 0,
    "gelu.small": lambda c: c["n"] in (4, 1020, 1024, 1028), "gelu.large": lambda c: c["n"] // 4 > 1 << 20 and c["n"] % 1024 != 0,
    "embed.vector": lambda c: embed_vector_route(c["patch"], c["E"]),
    "embed.nonsquare": lambda c: c["H"] != c["W"] and c["H"] // c["patch"] != c["W"] // c["patch"],
    "embed.p32": lambda c: c["patch"] == 32 and 3 * 32 * 32 // 4 > 256 and 3 * 32 * 32 + c["E"] > 1024 and embed_vector_route(c["patch"], c["E"]),
    "embed.f1024": lambda c: 3 * c["patch"] ** 2 < 1024 < 3 * c["patch"] ** 2 + c["E"] and embed_vector_route(c["patch"], c["E"]),
    "embed.scalar_patch": lambda c: c["E"] % 4 == 0 and not embed_vector_route(c["patch"], c["E"]),
    "embed.scalar_e": lambda c: c["patch"] % 4 == 0 and c["E"] % 4 != 0 and not embed_vector_route(c["patch"], c["E"]),
    "embed.e0": lambda c: c["E"] == 0,
    "embedb.cols32": lambda c: (c["P3"] + c["T"] * c["E"]) % 32 == 0,
    "embedb.e0": lambda c: c["E"] == 0, "embedb.acc": lambda c: c["acc"],
}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_shapes_have_the_property_their_label_claims(case):
    """GPU-free: per label, the chosen shape really reaches the branch under the launch selection as vit.hip spells it today."""
    for b in case.labels:
        if b in PROPERTY:
            assert PROPERTY[b](case), f"{case.id} does not have the property of {b}"
    if case.kind in ("afwd", "abwd", "acomp"):
        assert case["B"] <= 3 or (case["B"], case["T"]) == (5, 37), "B <= 3 except the shipped local-crop shape"
        assert case["heads"] in (1, 2, 3, 6)


def test_collective_shape_properties():
    """GPU-free: what a label asks of its cases together."""
    by = lambda label: [c for c in CASES if label in c.labels]
    kind = lambda k: [c for c in CASES if c.kind == k]
    fwd = kind("afwd")
    assert {c["T"] for c in fwd if not c["mode"] and not c["mult"]} == set(FWD_T)
    assert {c["heads"] for c in fwd} >= {1, 2, 3, 6} and {c["B"] for c in fwd} >= {1, 3}
    assert {c["layout"] for c in fwd} == set(_L3)
    for nw in ("fwd.nw2", "fwd.nw4"):                                  # every input mode and every layout in both kernel shapes
        assert {(c["mode"], c["mult"]) for c in by(nw)} >= {(None, 3), (None, 6), ("plant0", None), ("plantL", None), ("zero_q", None), ("dup", None)}, nw
        assert {c["layout"] for c in by(nw)} == set(_L3), nw
    assert {c["T"] for c in by("fwd.slab_skip")} >= {1, 5, 16, 33, 65, 97, 129, 161, 257} and {c["T"] for c in by("fwd.slab_both")} >= {17, 31, 32, 49, 64, 128, 256}
    assert {attn_fwd_plan(c["T"])["idle"] for c in by("fwd.wg2")} >= {0, 3}
    bwd = kind("abwd")
    for form, ts in BWD_T.items():
        have = [c for c in bwd if f"bwd.{form}" in c.labels]
        assert {c["T"] for c in have} >= set(ts), form
        assert {c["ldg"] for c in have} == {"fused", "dense", "padded"} and {c["ldo"] for c in have} == {"dense", "padded"} and {c["layout"] for c in have} == set(_L3), form
        assert {c["mult"] for c in have} >= {None, 3, 6} and {c["mode"] for c in have} >= {None, "plant0", "plantL"}, form
    assert {c["T"] for c in by("bwd.small_next")} >= {33, 37, 40} and {c["ldg"] for c in by("bwd.small_next")} == {"fused", "dense", "padded"}
    assert any(c["T"] == 41 and c["layout"] == "padded" for c in bwd) and any(c["T"] == 40 and c["layout"] == "padded" for c in bwd)
    assert any(c["ldg"] == "dense" and c["layout"] == "fused" for c in bwd), "ldg != ld"
    for form in ("fused2", "fused4", "fused8", "two_pass"):
        assert {c["mult"] for c in by(f"comp.{form}")} == {1, 3}, form
    ln = kind("ln")
    assert {c["M"] for c in ln if c["C"] == 384} >= set(LN_M) and {c["C"] for c in ln} >= set(LN_C)
    assert all(len({c["M"] for c in ln if c["C"] == ch}) >= 2 for ch in LN_C)
    for nit in ("ln.nit2", "ln.nit4", "ln.nit8"):
        assert {(bool(c["addend"]), bool(c["acc"])) for c in by(nit)} == {(a, b) for a in (False, True) for b in (False, True)}, nit
    assert {c["M"] for c in ln} >= {1, 8, 9, 31, 32, 33} and {ln_plan(c["M"], c["C"])["nblocks"] for c in ln} >= {1, 2, 3, 31, 33, 161}
    assert {c["B"] for c in by("embedb.chains")} >= {1, 7, 8, 9, 24, 25, 32, 33, 57}
    assert {bool(c["acc"]) for c in kind("embedb")} == {True, False} and any((c["P3"] + c["T"] * c["E"]) % 32 for c in kind("embedb"))
    assert {(c["H"], c["W"], c["patch"]) for c in kind("embed")} >= {(8, 16, 4), (16, 8, 4), (32, 96, 16), (64, 32, 32), (40, 80, 40)}
    assert any(c["patch"] == 6 and c["E"] == 8 for c in kind("embed")) and any(c["patch"] == 4 and c["E"] == 6 for c in kind("embed"))
    assert {embed_vector_route(c["patch"], c["E"]) for c in by("embed.e0")} == {True, False}
    sizes = {c["size"] for c in kind("crop")}
    assert sizes == {(7, 13), (32, 32), (1, 1)} and {15 * h * w % 256 == 0 for h, w in sizes} == {True, False}
    assert CROP_SRC[0] != CROP_SRC[1] and len(set(CROP_BOXES)) == 15
    hw = {(h, w) for _, _, h, w in CROP_BOXES}
    assert {h for h, _ in hw} >= {1, 2, 3, 24} and {w for _, w in hw} >= {1, 2, 3, 40} and (1, 1) in hw and (24, 40) in hw
    corners = {(t == 0, l == 0, t + h == CROP_SRC[0], l + w == CROP_SRC[1]) for t, l, h, w in CROP_BOXES}
    assert corners >= {(True, True, False, False), (True, False, False, True), (False, True, True, False), (False, False, True, True)}
    assert all(t >= 0 and l >= 0 and h >= 1 and w >= 1 and t + h <= CROP_SRC[0] and l + w <= CROP_SRC[1] for t, l, h, w in CROP_BOXES)


def _err(x, ref64):
    d = x.detach().double().cpu() - ref64
    return float(d.norm() / ref64.norm().clamp_min(1e-300)), float(d.abs().max() / ref64.abs().max().clamp_min(1e-300))


def _same(a, b):
    """bit-identical, a NaN equal to a NaN"""
    if not a.is_floating_point():
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_is_well_conditioned(case):
    """GPU-free, condition (b): the fp64 reference is finite and not identically zero, the fp32 evaluation of the same lines is within 1e-3 of it (e and
    m) and bit-identical for the family `exact`."""
    _, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    assert set(r64) == set(r32) and set(r64) <= set(FAMILY)
    assert r64 or case.kind == "refuse"
    for name, t in r64.items():
        if FAMILY[name] == "exact":
            assert _same(t.to(r32[name].dtype), r32[name]), f"{name}: the fp64 and fp32 references of an exact output differ"
            continue
        assert t.dtype == torch.float64 and r32[name].dtype == torch.float32, name
        assert torch.isfinite(t).all() and torch.isfinite(r32[name]).all(), name
        assert float(t.abs().max()) > 0, f"{name}: the reference is identically zero"
        e, m = _err(r32[name], t)
        print(f"{case.id} {name}: e(ref32) {e:.3e} m(ref32) {m:.3e}")
        assert e <= COND and m <= COND, f"{name}: ref32 is {e:.2e} / {m:.2e} from ref64 - the case measures nothing"
    if case.kind in ("afwd", "abwd", "acomp"):
        s = (_split(inp["q"].double(), case["B"], case["T"], case["heads"]) @ _split(inp["k"].double(), case["B"], case["T"], case["heads"]).transpose(-1, -2)) * _s(DH ** -0.5)
        print(f"{case.id}: largest |logit| {float(s.abs().max()):.1f}")
        if case["mult"] == 6:
            assert float(s.abs().max()) > 60.0, "the x 6 case does not reach large logits"
        if case["mode"] == "zero_q":
            assert float((r64["lse_f32"] - math.log(case["T"])).abs().max()) < 1e-12
    if case["mean"]:
        ratio = (inp["x"].mean(1) / inp["x"].std(1)).abs()                # 1000 nominal; a row's sample deviation wanders by a few per cent
        assert float(ratio.min()) > 800 and float(ratio.median()) > 950
    if case["const_row"]:
        assert float(r64["invstd"][0]) == 1.0 / math.sqrt(_s(LN_EPS)) and _same(r32["y"][0], inp["beta"])


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
    path = os.environ.get("SSV_VIT_REPORT")
    if path:
        blank = lambda: {"worst_e_ratio": 0.0, "worst_m_ratio": 0.0, "worst_e_case": "", "worst_m_case": ""}
        fams = {f: dict(blank(), FACTOR=FACTOR[f], FLOOR=FLOOR) for f in FACTOR}
        arith = {a: blank() for a in ARITH}                               # attention-forward, per arithmetic
        for cid, tensors in REPORT.items():
            for name, r in tensors.items():
                fam = FAMILY[name]
                rows = [fams[fam]] + ([arith[name.split("_", 1)[1]]] if fam == "attention-forward" else [])
                for k in ("e", "m"):
                    ratio = _ratio(r[f"{k}_got"], r[f"{k}_ref32"], FLOOR)
                    for row in rows:
                        if ratio > row[f"worst_{k}_ratio"]:
                            row[f"worst_{k}_ratio"], row[f"worst_{k}_case"] = ratio, f"{cid} {name}"
        with open(path, "w") as fh:
            json.dump({"source_sha16": _lib().source_sha16(), "families": fams, "attention_forward_by_arithmetic": arith, "cases": REPORT}, fh, indent=1, sort_keys=True)


class Ctx:
    """The device side of one run of one case: uploaded inputs (kept to prove them untouched), guarded outputs, stated identities."""

    def __init__(self, dev):
        self.dev, self.ins, self.bufs, self.mats, self.same = dev, [], [], [], []

    def up(self, name, t):
        """an input, 16-byte aligned, with at least GUARD elements of slack behind it: a kernel that over-reads by a row fails its case, it does not fault"""
        buf = torch.zeros((t.numel() + max(GUARD, t.shape[-1] if t.dim() else 0),), dtype=t.dtype, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        d = buf[:t.numel()].view(t.shape)
        d.copy_(t)
        self.ins.append((name, d, d.clone()))
        return d

    def place(self, name, tensors, layout, pad=4):
        """[M, hid] operands as the layout asks: column blocks of one matrix (fused), own dense buffers, or own buffers with `pad` NaN columns per row"""
        hid = tensors[0].shape[1]
        if layout == "fused":
            d = self.up(name, torch.cat(tensors, 1))
            return [d[:, i * hid:(i + 1) * hid] for i in range(len(tensors))]
        if layout == "dense":
            return [self.up(f"{name}[{i}]", t) for i, t in enumerate(tensors)]
        out = []
        for i, t in enumerate(tensors):
            full = torch.full((t.shape[0], hid + pad), float("nan"))
            full[:, :hid] = t
            out.append(self.up(f"{name}[{i}]", full)[:, :hid])
        return out

    def out(self, name, shape, prior=None, nan_ok=False, guard=GUARD, shift=0):
        """a 16-byte aligned view (shift: offset in floats from such a view) into a NaN-prefilled buffer: the payload is rounded up to a multiple of 4 floats before the guard"""
        n = math.prod(shape)
        buf = torch.full((shift + (n + 3) // 4 * 4 + guard,), float("nan"), device=self.dev)
        assert buf.data_ptr() % 16 == 0
        if prior is not None:
            buf[shift:shift + n].copy_(prior.reshape(-1))
        self.bufs.append((name, buf, shift, n, nan_ok))
        return buf[shift:shift + n].view(shape)

    def mat(self, name, rows, width, blocks):
        """a NaN-prefilled [rows, width] matrix of which only the column blocks (first column, columns) are outputs: (the blocks' views, width)"""
        full = self.out(name, (rows, width), nan_ok=True)
        self.mats.append((name, full, blocks))
        return [full[:, c0:c0 + n] for c0, n in blocks], width

    def grads(self, name, rows, hid, layout):
        """dq, dk, dv and ldg"""
        if layout == "fused":
            return self.mat(name, rows, 3 * hid, [(i * hid, hid) for i in range(3)])
        if layout == "padded":
            return self.mat(name, rows, 3 * hid + 12, [(i * (hid + 4), hid) for i in range(3)])
        return [self.mat(f"{name}[{i}]", rows, hid, [(0, hid)])[0][0] for i in range(3)], hid

    def ws(self, name, nbytes):
        nbytes = int(nbytes)
        assert nbytes % 4 == 0
        return self.out(name, (nbytes // 4,), nan_ok=True, guard=WS_GUARD), nbytes

    def verify(self, what):
        torch.cuda.synchronize()
        for name, d, keep in self.ins:
            assert _same(d, keep), f"{what}: input {name} was modified"
        for name, buf, shift, n, nan_ok in self.bufs:
            assert nan_ok or not torch.isnan(buf[shift:shift + n]).any(), f"{what} {name}: {int(torch.isnan(buf[shift:shift + n]).sum())} elements never written (or NaN)"
            assert torch.isnan(buf[shift + n:]).all() and torch.isnan(buf[:shift]).all(), f"{what} {name}: wrote outside its view"
        for name, full, blocks in self.mats:
            keep = torch.ones(full.shape[1], dtype=torch.bool, device=self.dev)
            for c0, n in blocks:
                keep[c0:c0 + n] = False
                assert not torch.isnan(full[:, c0:c0 + n]).any(), f"{what} {name}: columns {c0}..{c0 + n} hold {int(torch.isnan(full[:, c0:c0 + n]).sum())} elements never written (or NaN)"
            assert torch.isnan(full[:, keep]).all(), f"{what} {name}: wrote into its padding columns"
        for name, a, b in self.same:
            assert _same(a, b), f"{what}: {name} not bit-identical (max |diff| {float((a.double() - b.double()).abs().max()):.3e})"


def _refused(fn, *args):
    """the call returns an error status (raised as SsvError by _lib.call): nothing was launched"""
    L = _lib()
    with pytest.raises(L.SsvError):
        L.call(fn, *args)


SCALE = DH ** -0.5


def _fwd_call(ctx, c, q, k, v, ldo_pad, arith, tag):
    """one forward launch: (o [M, hid] view, lse); arith None: through ssv_attention_fwd"""
    L = _lib()
    P = L.ptr
    b, t, h = c["B"], c["T"], c["heads"]
    hid = h * DH
    (o,), ldo = ctx.mat(f"o {tag}", b * t, hid + ldo_pad, [(0, hid)])
    lse = ctx.out(f"lse {tag}", (b, h, t))
    ld = q.stride(0)
    assert ld == k.stride(0) == v.stride(0)
    if arith is None:
        L.call("ssv_attention_fwd", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(o), ldo, P(lse), L.stream())
    else:
        L.call("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(o), ldo, P(lse), ARITH[arith], L.stream())
    return o, lse


def _afwd_gpu(c, inp, ctx):
    layout = c["layout"]
    q, k, v = ctx.place("qkv", [inp["q"], inp["k"], inp["v"]], layout)
    pad = 8 if layout == "padded" else 0
    out = {}
    for a in ARITH:
        o, lse = _fwd_call(ctx, c, q, k, v, pad, a, a)
        o2, lse2 = _fwd_call(ctx, c, q, k, v, pad, a, a + " again")
        ctx.same += [(f"{a}, second call: o", o, o2), (f"{a}, second call: lse", lse, lse2)]
        if layout == "fused":                                           # (d): dense operands give the bits of the strided slices
            qd, kd, vd = ctx.place("qkv dense", [inp["q"], inp["k"], inp["v"]], "dense")
            o3, lse3 = _fwd_call(ctx, c, qd, kd, vd, 0, a, a + " dense")
            ctx.same += [(f"{a}, dense vs strided: o", o, o3), (f"{a}, dense vs strided: lse", lse, lse3)]
        out.update({f"o_{a}": o, f"lse_{a}": lse})
    o4, lse4 = _fwd_call(ctx, c, q, k, v, pad, None, "ssv_attention_fwd")
    ctx.same += [("ssv_attention_fwd vs ssv_attention_fwd_arith(F32_MFMA): o", o4, out["o_f32"]), ("... lse", lse4, out["lse_f32"])]
    return out


def _bwd_call(ctx, c, q, k, v, o, dout, lse, ldg_layout, tag):
    L = _lib()
    P = L.ptr
    b, t, h = c["B"], c["T"], c["heads"]
    (dq, dk, dv), ldg = ctx.grads(f"grads {tag}", b * t, h * DH, ldg_layout)
    delta = ctx.out(f"delta {tag}", (b, h, t))
    assert o.stride(0) == dout.stride(0)
    L.call("ssv_attention_bwd", b, t, h, DH, P(q), P(k), P(v), q.stride(0), SCALE, P(o), P(dout), o.stride(0), P(lse), P(delta), P(dq), P(dk), P(dv), ldg, L.stream())
    return {"delta": delta, "dq": dq, "dk": dk, "dv": dv}


def _abwd_gpu(c, inp, ctx):
    q, k, v = ctx.place("qkv", [inp["q"], inp["k"], inp["v"]], c["layout"])
    o, dout = ctx.place("o, dout", [inp["o_in"], inp["dout"]], c["ldo"], pad=8)
    lse = ctx.up("lse", inp["lse_in"])
    got = _bwd_call(ctx, c, q, k, v, o, dout, lse, c["ldg"], "")
    again = _bwd_call(ctx, c, q, k, v, o, dout, lse, c["ldg"], "again")
    ctx.same += [(f"ssv_attention_bwd, second call: {n}", got[n], again[n]) for n in got]
    other = _bwd_call(ctx, c, q, k, v, o, dout, lse, "dense" if c["ldg"] != "dense" else "padded", "other ldg")
    ctx.same += [(f"ssv_attention_bwd, another gradient layout: {n}", got[n], other[n]) for n in got]
    if c["T"] == 1:
        # one key: P = exp(s - lse) = 1 up to lse's rounding and dout . v - delta is zero up to the two sums' roundings, each at most 64 U sum|dout_d v_d|.
        # So |dS| <= 2 * 64 U * sum|dout_d v_d| (P <= 1 + 2^-10 at these logits), |dq_d| <= scale |dS| |k_d| and |dk_d| <= scale |dS| |q_d|
        b, h = c["B"], c["heads"]
        ds = 1.001 * 128 * U * (inp["dout"].double().abs() * inp["v"].double().abs()).view(b, h, DH).sum(-1, keepdim=True)
        for name, other_op in (("dq", "k"), ("dk", "q")):
            bound = (_s(SCALE) * ds * inp[other_op].double().abs().view(b, h, DH)).view(b, h * DH)
            g = got.pop(name).cpu().double()
            assert bool((g.abs() <= bound).all()), f"T = 1: |{name}| up to {float(g.abs().max()):.3e}, bound {float(bound.max()):.3e}"
    return got


def _acomp_gpu(c, inp, ctx):
    q, k, v = ctx.place("qkv", [inp["q"], inp["k"], inp["v"]], "fused")
    dout = ctx.up("dout", inp["dout"])
    out = {}
    for a in ARITH:
        o, lse = _fwd_call(ctx, c, q, k, v, 0, a, a)
        got = _bwd_call(ctx, c, q, k, v, o, dout, lse, "fused", a)
        out.update({f"{n}_{a}": got[n] for n in ("dq", "dk", "dv")})
    return out


def _ln_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    m, ch = c["M"], c["C"]
    x, gamma, beta, dy, mean_in, invstd_in = (ctx.up(n, inp[n]) for n in ("x", "gamma", "beta", "dy", "mean_in", "invstd_in"))
    addend = ctx.up("addend", inp["addend"]) if c["addend"] else None
    dx_addend = ctx.up("dx_addend", inp["dx_addend"]) if c["addend"] else None

    def fwd(add, tag):
        y, mean, invstd = ctx.out("y" + tag, (m, ch)), ctx.out("mean" + tag, (m,)), ctx.out("invstd" + tag, (m,))
        L.call("ssv_layernorm_fwd", m, ch, P(x), P(gamma), P(beta), P(add), LN_EPS, P(y), P(mean), P(invstd), L.stream())
        return {"y": y, "mean": mean, "invstd": invstd}
    out, again = fwd(addend, ""), fwd(addend, " again")
    ctx.same += [(f"ssv_layernorm_fwd, second call: {n}", out[n], again[n]) for n in out]
    if c["addend"]:
        plain = fwd(None, " (no addend)")
        ctx.same += [(f"ssv_layernorm_fwd without addend: {n}", out[n], plain[n]) for n in ("mean", "invstd")]
    wsb = L.load().ssv_layernorm_workspace_bytes(m, ch)
    assert wsb == ln_plan(m, ch)["ws_bytes"], "ln_plan as restated in this file is not the library's"

    def bwd(mode, tag, inplace=False):
        pri = {"ow": (None, None), "acc": (inp["dg0"], inp["db0"]), "zero": (torch.zeros(ch), torch.zeros(ch))}[mode]
        dg, db = ctx.out("dgamma" + tag, (ch,), prior=pri[0]), ctx.out("dbeta" + tag, (ch,), prior=pri[1])
        dx = ctx.out("dx" + tag, (m, ch), prior=inp["dx_addend"] if inplace else None)
        ws, _ = ctx.ws("workspace" + tag, wsb)
        L.call("ssv_layernorm_bwd", m, ch, P(dy), P(x), P(gamma), P(mean_in), P(invstd_in), P(dx) if inplace else P(dx_addend), P(dx), P(dg), P(db),
               int(mode != "ow"), P(ws), wsb, L.stream())
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    mode = "acc" if c["acc"] else "ow"
    got, again = bwd(mode, ""), bwd(mode, " again")
    ctx.same += [(f"ssv_layernorm_bwd, second call: {n}", got[n], again[n]) for n in got]
    zero, plain = bwd("zero", " zero prior"), bwd("ow", " overwrite")
    ctx.same += [(f"ssv_layernorm_bwd, accumulate on a zero prior vs overwrite: {n}", zero[n], plain[n]) for n in zero]
    if c["addend"]:
        inplace = bwd(mode, " in place", inplace=True)
        ctx.same += [(f"ssv_layernorm_bwd in place (dx_addend == dx): {n}", got[n], inplace[n]) for n in got]
    out.update(got)
    return out


def _gelu_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    n = c["n"]
    x, dy = ctx.up("x", inp["x"]), ctx.up("dy", inp["dy"])
    y, dx = ctx.out("gelu_y", (n,)), ctx.out("gelu_dx", (n,))
    L.call("ssv_gelu_fwd", n, P(x), P(y), L.stream())
    L.call("ssv_gelu_bwd", n, P(x), P(dy), P(dx), L.stream())
    return {"gelu_y": y, "gelu_dx": dx}


def _embed_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    b, h, w, patch, e = c["B"], c["H"], c["W"], c["patch"], c["E"]
    t, f = (h // patch) * (w // patch) + 1, 3 * patch * patch + e
    img, cls = ctx.up("img", inp["img"].permute(0, 2, 3, 1).contiguous()), ctx.up("cls", inp["cls"])
    pos = ctx.up("pos", inp["pos"] if e else torch.zeros(4))             # E = 0: a pointer nobody reads
    tok = ctx.out("tok", (b * t, f))
    L.call("ssv_vit_embed_fwd", b, h, w, patch, e, P(img), P(cls), P(pos), P(tok), L.stream())
    off = ctx.out("tok (+ 4 bytes)", (b * t, f), shift=1)                # a misaligned token pointer: the scalar kernel
    assert off.data_ptr() % 16 == 4 and not embed_vector_route(patch, e, aligned=False)
    L.call("ssv_vit_embed_fwd", b, h, w, patch, e, P(img), P(cls), P(pos), P(off), L.stream())
    ctx.same.append(("ssv_vit_embed_fwd, aligned vs offset token pointer (vector vs scalar kernel where eligible)", tok, off))
    return {"tok": tok}


def _embedb_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    b, t, p3, e = c["B"], c["T"], c["P3"], c["E"]
    dtok = ctx.up("dtok", inp["dtok"])

    def run(mode, tag):
        pri = {"ow": (None, None), "acc": (inp["dcls0"], inp["dpos0"]), "zero": (torch.zeros(p3), torch.zeros(t + 2, e))}[mode]
        dcls = ctx.out("dcls" + tag, (p3,), prior=pri[0])
        dpos = ctx.out("dpos" + tag, (t + 2, max(e, 1)), nan_ok=True)   # two rows past T (and with E = 0 a buffer nobody may write)
        if pri[1] is not None and e:
            dpos[:t].copy_(pri[1][:t])
        L.call("ssv_vit_embed_bwd", b, t, p3, e, P(dtok), P(dcls), P(dpos), int(mode != "ow"), L.stream())
        torch.cuda.synchronize()
        assert torch.isnan(dpos[t:]).all(), "rows of dpos past T were written"
        assert not torch.isnan(dpos[:t]).any() if e else torch.isnan(dpos).all(), "dpos: rows never written, or written with E = 0"
        return {"dcls": dcls, "dpos": dpos[:t]} if e else {"dcls": dcls}
    mode = "acc" if c["acc"] else "ow"
    got, again = run(mode, ""), run(mode, " again")
    ctx.same += [(f"ssv_vit_embed_bwd, second call: {n}", got[n], again[n]) for n in got]
    zero, plain = run("zero", " zero prior"), run("ow", " overwrite")
    ctx.same += [(f"ssv_vit_embed_bwd, accumulate on a zero prior vs overwrite: {n}", zero[n], plain[n]) for n in zero]
    return got


def _crop_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    ho, wo = c["size"]
    views, boxes = ctx.up("views", inp["views"]), ctx.up("boxes", inp["boxes"])
    out = ctx.out("crop", (3, 5, ho, wo, 3))
    L.call("ssv_multicrop", 3, CROP_SRC[0], CROP_SRC[1], P(views), 5, P(boxes), ho, wo, P(out), L.stream())
    if "crop.oracle" in c.labels:
        from oracle import vit as ovit
        for b in range(3):
            for j in range(5):
                want = ovit.multicrop_resize(inp["views"][b].permute(2, 0, 1), tuple(int(x) for x in inp["boxes"][b, j]), (ho, wo))
                torch.testing.assert_close(out[b, j].permute(2, 0, 1).cpu(), want, rtol=1e-4, atol=2e-5, msg=f"box {CROP_BOXES[b * 5 + j]} against torch's bicubic interpolate")
    return {"crop": out}


def _refuse_gpu(c, inp, ctx):
    L = _lib()
    P = L.ptr
    what = c["what"]
    g = c.gen()
    s = L.stream()
    if what in ("dh32", "ld_mod4", "ld_short", "misaligned", "arithmetic"):
        b, t, h, hid = 2, 5, 2, 128
        src = ctx.up("qkv", _rn(g, b * t + 1, 3 * hid + 8))
        q, k, v = src[:b * t, :hid], src[:b * t, hid:2 * hid], src[:b * t, 2 * hid:3 * hid]
        o, dout, lse = ctx.up("o", _rn(g, b * t, hid)), ctx.up("dout", _rn(g, b * t, hid)), ctx.up("lse", _rn(g, b, h, t))
        outs = [ctx.out(n, (b * t + 1, hid + 4), nan_ok=True) for n in ("o out", "dq", "dk", "dv")] + [ctx.out(n, (b, h, t), nan_ok=True) for n in ("lse out", "delta")]
        oo, dq, dk, dv, lo, delta = outs
        ld = src.stride(0)
        if what == "dh32":
            _refused("ssv_attention_fwd_arith", b, t, 4, 32, P(q), P(k), P(v), ld, SCALE, P(oo), hid, P(lo), ARITH["f32"], s)
            _refused("ssv_attention_bwd", b, t, 4, 32, P(q), P(k), P(v), ld, SCALE, P(o), P(dout), hid, P(lse), P(delta), P(dq), P(dk), P(dv), hid, s)
        if what == "ld_mod4":
            for a in ARITH.values():
                _refused("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k), P(v), ld - 2, SCALE, P(oo), hid, P(lo), a, s)
                _refused("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(oo), hid + 2, P(lo), a, s)
            _refused("ssv_attention_bwd", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(o), P(dout), hid, P(lse), P(delta), P(dq), P(dk), P(dv), hid + 2, s)
        if what == "ld_short":
            _refused("ssv_attention_bwd", b, t, h, DH, P(q), P(k), P(v), hid - 4, SCALE, P(o), P(dout), hid, P(lse), P(delta), P(dq), P(dk), P(dv), hid, s)
            _refused("ssv_attention_bwd", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(o), P(dout), hid, P(lse), P(delta), P(dq), P(dk), P(dv), hid - 4, s)
            _refused("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k), P(v), hid - 4, SCALE, P(oo), hid, P(lo), ARITH["bf16x3"], s)
        if what == "misaligned":
            _refused("ssv_attention_fwd", b, t, h, DH, P(q) + 4, P(k), P(v), ld, SCALE, P(oo), hid, P(lo), s)
            _refused("ssv_attention_fwd", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(oo) + 4, hid, P(lo), s)
            _refused("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k) + 4, P(v), ld, SCALE, P(oo), hid, P(lo), ARITH["bf16x3"], s)
            _refused("ssv_attention_bwd", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(o), P(dout), hid, P(lse), P(delta), P(dq), P(dk) + 4, P(dv), hid, s)
        if what == "arithmetic":
            for a in (1, 5, 7, -1):
                _refused("ssv_attention_fwd_arith", b, t, h, DH, P(q), P(k), P(v), ld, SCALE, P(oo), hid, P(lo), a, s)
    elif what in ("ln_c6", "ln_c2052", "ln_ws"):
        m, ch = 5, {"ln_c6": 6, "ln_c2052": 2052, "ln_ws": 384}[what]
        x, gamma, dy, mean, invstd = ctx.up("x", _rn(g, m, ch)), ctx.up("gamma", _rn(g, ch)), ctx.up("dy", _rn(g, m, ch)), ctx.up("mean", _rn(g, m)), ctx.up("invstd", _rn(g, m))
        outs = [ctx.out(n, shape, nan_ok=True) for n, shape in (("y", (m, ch)), ("mean out", (m,)), ("invstd out", (m,)), ("dx", (m, ch)), ("dgamma", (ch,)), ("dbeta", (ch,)))]
        y, mo, io, dx, dg, db = outs
        wsb = 2 * ch * 4
        ws, _ = ctx.ws("workspace", wsb + 4)
        outs.append(ws)
        if what != "ln_ws":
            _refused("ssv_layernorm_fwd", m, ch, P(x), P(gamma), P(gamma), None, LN_EPS, P(y), P(mo), P(io), s)
            _refused("ssv_layernorm_bwd", m, ch, P(dy), P(x), P(gamma), P(mean), P(invstd), None, P(dx), P(dg), P(db), 0, P(ws), wsb + 4, s)
        else:
            assert L.load().ssv_layernorm_workspace_bytes(m, ch) == wsb
            _refused("ssv_layernorm_bwd", m, ch, P(dy), P(x), P(gamma), P(mean), P(invstd), None, P(dx), P(dg), P(db), 0, P(ws), wsb - 1, s)
    elif what == "gelu_n6":
        x = ctx.up("x", _rn(g, 8))
        outs = [ctx.out("y", (8,), nan_ok=True), ctx.out("dx", (8,), nan_ok=True)]
        _refused("ssv_gelu_fwd", 6, P(x), P(outs[0]), s)
        _refused("ssv_gelu_bwd", 6, P(x), P(x), P(outs[1]), s)
    else:
        assert what == "embed_ragged"
        img, cls, pos = ctx.up("img", _rn(g, 2, 10, 8, 3)), ctx.up("cls", _rn(g, 48)), ctx.up("pos", _rn(g, 8, 4))
        outs = [ctx.out("tok", (2 * 8, 52), nan_ok=True)]
        _refused("ssv_vit_embed_fwd", 2, 10, 8, 4, 4, P(img), P(cls), P(pos), P(outs[0]), s)
        _refused("ssv_vit_embed_fwd", 2, 8, 10, 4, 4, P(img), P(cls), P(pos), P(outs[0]), s)
    torch.cuda.synchronize()
    for o_ in outs:
        assert bool(torch.isnan(o_).all()), "a refused call wrote an output"
    return {}


GPU = {"afwd": _afwd_gpu, "abwd": _abwd_gpu, "acomp": _acomp_gpu, "ln": _ln_gpu, "gelu": _gelu_gpu, "embed": _embed_gpu, "embedb": _embedb_gpu, "crop": _crop_gpu,
       "refuse": _refuse_gpu}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_kernel_against_fp64(dev, case):
    _, make, ref = KINDS[case.kind]
    inp = make(case)
    r64, r32 = ref(case, inp, torch.float64), ref(case, inp, torch.float32)
    ctx = Ctx(dev)
    got = GPU[case.kind](case, inp, ctx)
    torch.cuda.synchronize()
    assert set(got) == set(r64), f"{case.id}: {sorted(set(got) ^ set(r64))}"
    fails, rec = [], REPORT.setdefault(case.id, {})
    for name, ref64 in r64.items():
        g = got[name].detach().reshape(ref64.shape).cpu()
        fam = FAMILY[name]
        if fam == "exact":
            if not _same(g, r32[name]):
                fails.append(f"{case.id} {name}: not bit-identical to the reference ({int((g != r32[name]).sum())} of {g.numel()} elements differ)")
            continue
        assert torch.isfinite(g).all(), f"{case.id} {name}: non-finite values"
        (eg, mg), (er, mr) = _err(g, ref64), _err(r32[name], ref64)
        rec[name] = {"e_got": eg, "e_ref32": er, "m_got": mg, "m_ref32": mr}
        print(f"{case.id} {name}: e {eg:.3e} (ref32 {er:.3e}) m {mg:.3e} (ref32 {mr:.3e})")
        if not (eg <= FACTOR[fam] * er + FLOOR and mg <= FACTOR[fam] * mr + FLOOR):
            fails.append(f"{case.id} {name}: e {eg:.3e} vs ref32 {er:.3e}, m {mg:.3e} vs ref32 {mr:.3e} (FACTOR {FACTOR[fam]:g}, FLOOR {FLOOR:.2e})")
    ctx.verify(case.id)
    assert not fails, "\n".join(fails)
