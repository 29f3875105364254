// ProtoNCE, the prototype term of Prototypical Contrastive Learning (Li, Zhou, Xiong, Hoi, ICLR 2021): every query against `segs` sets of prototypes, each
// prototype with its own inverse concentration.  The contract is in include/ssv_hip.h (ssv_proto_nce).  The prototypes carry no gradient, so the loss and
// d loss / d q together are ONE pass of the shape of a flash-attention forward: scores S = (Q C^T) o inv_phi, values V = inv_phi o C, output softmax(S) V minus
// the positive's row of V.
//
//   * SSV_ARITH_BF16X3, d % 32 == 0, d <= SSV_PROTO_NCE_FUSED_MAX_D: FUSED (pn_fused_k).  S and P never reach memory.  The pass is written once, as the text of csrc/bank_softmax_pass.h
//     (included here with the source Segments; qn_fused_k of csrc/densecl.hip includes it with the source Range), and described here.  The operand plan is nn_fused_k's
//     (csrc/nnlookup.hip): the prototypes are streamed in fp32 and split in registers as the A operand of v_mfma_f32_32x32x16_bf16, the queries are split once
//     per call into fragment order (pn_prep_k) and are the B operand, so a LANE owns a QUERY: element r of the score tile in lane (c, h) is query c against
//     prototype acc32_row(r, h) of the tile, and the running max and sum are compare, exp and add inside the lane (one exchange with lane ^ 32 per tile for the
//     max, which both halves must share because they share the output accumulators).  The second product out^T += V^T P^T runs on the same instruction with the
//     QUERIES still the B operand: lane (c, h) supplies as contraction slots 8 h .. 8 h + 7 of slab u its own accumulator elements 8 u .. 8 u + 7 - the
//     prototypes (i & 3) + 16 u + 8 (i >> 2) + 4 h - and the A operand (lane (dd, h): column 32 dt + dd of V) is read from LDS IN THAT ORDER, so P goes from the
//     accumulator layout into the instruction without a shuffle.  The tile of scaled prototypes is written to LDS (per wave, 16-byte granules XOR-swizzled by
//     the row) while the first product streams it, and read back transposed.  P and V are split into bf16 pieces like every other operand (split_bf16.h).
//     A workgroup owns one slice of one segment (L rows, a multiple of SSV_PROTO_NCE_SLICE) and one block of KT query tiles; its four waves take the four
//     quarters of the slice and each leaves (max, sum, acc[d]) in the workspace.  pn_fold_k merges the quarters of all slices of a segment in ascending order,
//     then the segments in ascending order, subtracts the positive rows and writes lse and dq; pn_loss_k sums the per-row losses in a fixed order.
//     The positive's score is caught inside the fused kernel (the one lane that holds it stores it), so lse - s_y is a difference of two values of ONE
//     instruction sequence: a one-prototype segment gives exactly lse = s_y and a zero loss (its p v - v is v's accumulator roundings, not an exact zero).
//     Numerics of both routes: the running maximum and lse take the ROUNDED score (the contract's one fp32 multiply), the exponents take the unrounded product
//     through an fma - rounding a score of magnitude 20 would cost every p 1e-6 - and the row loss is log(sum) + (max - s_y), never (max + log(sum)) - s_y.
//   * SSV_ARITH_F32_MFMA, or another width: UNFUSED, per segment and chunk of queries: the segment is copied behind zero rows to a multiple of 16 (pn_pad_k: the
//     data-gradient GEMM contracts whole 16-row groups, and no row behind ktot is ever read), S on ssv_conv2d_fwd, one wavefront per row scales, reduces and
//     overwrites S with d loss / d S (pn_row_k), ssv_conv2d_dgrad accumulates dq.  The softmax-CE kernel of the linear probe returns a mean and no lse, so the
//     row kernel is this file's own.
// No floating-point atomics anywhere; every workspace value that is read was written by the same call.
#include "bank_softmax.h"

namespace {

using banksm::arith_ok;
using banksm::mul_rn;

constexpr int SLICE = SSV_PROTO_NCE_SLICE, MAX_SLICES = SSV_PROTO_NCE_MAX_SLICES, FUSED_MAX_D = SSV_PROTO_NCE_FUSED_MAX_D;
constexpr int MAX_M = SSV_PROTO_NCE_MAX_M, MAX_SEGS = SSV_PROTO_NCE_MAX_SEGS, MAX_D = SSV_KNN_MAX_D;

struct SegTab {                                       // by value into every kernel: no table in device memory, nothing to upload
  int begin[MAX_SEGS], end[MAX_SEGS];                 // prototype rows [begin, end) of the segment
  int rows[MAX_SEGS], first[MAX_SEGS + 1];            // fused: rows of one slice, index of the segment's first slice (first[segs] = all slices)
  int segs;
};

struct Plan : banksm::FusedPlan {
  bool fused;
  int64_t max_slices;                                 // fused: slices of the worst segmentation of ktot rows into segs segments
  int cr; int64_t kp;                                 // unfused: query rows of a chunk, rows of the longest possible segment rounded up to 16
  size_t spos_bytes, rl_bytes, s_bytes, cpad_bytes;
  size_t total() const { return spos_bytes + rl_bytes + 2 * pm_bytes + pacc_bytes + planes_bytes + s_bytes + cpad_bytes; }
};

bool shape_ok(int32_t m, int64_t ktot, int32_t d, int32_t segs) {
  return m >= 1 && m <= MAX_M && segs >= 1 && segs <= MAX_SEGS && ktot >= segs && ktot < (1ll << 31) && d >= 4 && d <= MAX_D && d % 4 == 0;
}

Plan make_plan(int32_t m, int64_t ktot, int32_t d, int32_t segs, int32_t arithmetic) {
  Plan p = {};
  p.fused = arithmetic == SSV_ARITH_BF16X3 && d % 32 == 0 && d <= FUSED_MAX_D;
  p.spos_bytes = up256((size_t)segs * ((m + 31) / 32 * 32) * 4);
  p.rl_bytes = up256((size_t)segs * m * 4);
  if (p.fused) {
    banksm::plan_tiles(p, m, d);
    const int64_t by_rows = cdiv64(ktot, SLICE) + segs, by_cap = (int64_t)MAX_SLICES * segs;
    p.max_slices = by_rows < by_cap ? by_rows : by_cap;
    banksm::plan_bytes(p, p.max_slices, d);
  } else {
    p.mpad = m;
    p.kp = (ktot - (segs - 1) + 15) / 16 * 16;
    p.cr = banksm::chunk_rows(p.kp, m);
    p.s_bytes = up256((size_t)p.cr * p.kp * 4);
    p.cpad_bytes = up256((size_t)p.kp * d * 4);
  }
  return p;
}

// ---- both routes: bad device data --------------------------------------------------------------------------------------------------------------------------
// bit 0: a label outside its segment; bit 1: an inv_phi that is not finite and positive.  Integer atomics only.
__global__ void __launch_bounds__(256) pn_check_k(SegTab tab, int m, int64_t ktot, const float* __restrict__ inv_phi, const int32_t* __restrict__ labels,
                                                  int32_t* __restrict__ flag) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int bad = 0;
  if (u < ktot) {
    const float v = inv_phi[u];
    if (!(v > 0.f && v < INFINITY)) bad |= 2;
  }
  if (u < (int64_t)tab.segs * m) {
    const int s = (int)(u / m);
    if ((unsigned)labels[u] >= (unsigned)(tab.end[s] - tab.begin[s])) bad |= 1;
  }
  if (bad) atomicOr(flag, bad);
}

// the per-row losses rl [n] in a fixed order: thread t takes t, t + 256, ..., then the fixed tree
__global__ void __launch_bounds__(256) pn_loss_k(int n, const float* __restrict__ rl, float scale, float* __restrict__ loss) {
  __shared__ float sm[256];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += rl[i];
  sm[threadIdx.x] = a;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) loss[0] = sm[0] * scale;
}

// ---- fused ---------------------------------------------------------------------------------------------------------------------------------------------------
// the queries' three planes in fragment order with d / 16 slabs (banksm::prep_planes); rows behind m are zeros
__global__ void __launch_bounds__(256) pn_prep_k(int d, int m, int T, int NS, const float* __restrict__ q, u32x4* __restrict__ planes) {
  banksm::prep_planes<false>(d, m, T, NS, q, planes);
}

// the pass of bank_softmax_pass.h over one slice of one segment: the slice's segment from the table, then the pass with the segment's scales, labels and positives
template <int DT, int KT>
__global__ void __launch_bounds__(256, 1)
pn_fused_k(const float* __restrict__ protos, const float* __restrict__ inv_phi, const int32_t* __restrict__ labels, SegTab tab, int m, int T, int mpad,
           const u32x4* __restrict__ planes, float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ pacc, float* __restrict__ spos) {
  constexpr int D = 32 * DT;
  __shared__ float vt[4][32 * D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int tb = blockIdx.y * KT, sl = blockIdx.x;
  int seg = 0;
#pragma unroll
  for (int k = 1; k < MAX_SEGS; ++k) seg = (k < tab.segs && sl >= tab.first[k]) ? k : seg;
  const int64_t seg_b = tab.begin[seg], end = tab.end[seg], L = tab.rows[seg];
  const auto slice0 = [&] { return seg_b + (int64_t)(sl - tab.first[seg]) * L; };      // evaluated where the pass needs it
  const float* bank = protos;
  using SRC = banksm::Segments;
  const SRC src = {inv_phi, labels, spos, seg, seg_b, m, 0.f};
#include "bank_softmax_pass.h"
}

// one wavefront per query: per segment the partials in ascending order, the positive's row off, then the segments in ascending order
__global__ void __launch_bounds__(256) pn_fold_k(SegTab tab, int m, int d, int mpad, const float* __restrict__ pm, const float* __restrict__ pl,
                                                 const float* __restrict__ pacc, const float* __restrict__ spos, const float* __restrict__ protos,
                                                 const float* __restrict__ inv_phi, const int32_t* __restrict__ labels, float inv, float* __restrict__ lse,
                                                 float* __restrict__ rl, float* __restrict__ dq) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= m) return;
  constexpr int NE = FUSED_MAX_D / 64;
  float g[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) g[k] = 0.f;
  for (int s = 0; s < tab.segs; ++s) {
    const int p0 = 4 * tab.first[s], p1 = 4 * tab.first[s + 1];
    float M = -INFINITY;
    for (int p = p0; p < p1; ++p) M = fmaxf(M, pm[(int64_t)p * mpad + i]);
    float Ls = 0.f, a[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) a[k] = 0.f;
    for (int p = p0; p < p1; ++p) {
      const int64_t o = (int64_t)p * mpad + i;
      const float mp = pm[o];
      const float w = mp == -INFINITY ? 0.f : expf(mp - M);               // a quarter behind the segment's end holds (-inf, 0, 0)
      Ls += pl[o] * w;
#pragma unroll
      for (int k = 0; k < NE; ++k)
        if (lane + 64 * k < d) a[k] += pacc[o * d + lane + 64 * k] * w;
    }
    const int ks = tab.end[s] - tab.begin[s];
    int y = labels[(int64_t)s * m + i];
    y = y < 0 ? 0 : (y >= ks ? ks - 1 : y);                              // out of range: reported by pn_check_k, never dereferenced
    const int64_t row = (int64_t)tab.begin[s] + y;
    const float ipy = inv_phi[row];
#pragma unroll
    for (int k = 0; k < NE; ++k)
      if (lane + 64 * k < d) g[k] += a[k] / Ls - mul_rn(protos[row * d + lane + 64 * k], ipy);     // the rounded product pn_fused_k staged, not an fma's exact one
    if (lane == 0) {
      const float lg = logf(Ls);
      lse[(int64_t)s * m + i] = M + lg;
      rl[(int64_t)s * m + i] = lg + (M - spos[(int64_t)s * mpad + i]);     // not (M + lg) - s_y: the sum would be rounded at lse's magnitude before the difference
    }
  }
#pragma unroll
  for (int k = 0; k < NE; ++k)
    if (lane + 64 * k < d) dq[(int64_t)i * d + lane + 64 * k] = g[k] * inv;
}

// ---- unfused -------------------------------------------------------------------------------------------------------------------------------------------------
// rows [0, k) of a segment into dst [kp][d], zero rows behind k
__global__ void __launch_bounds__(256) pn_pad_k(int64_t k, int64_t kp, int d4, const f32x4* __restrict__ src, f32x4* __restrict__ dst) {
  banksm::pad_rows(k, kp, d4, src, dst);
}

// one wavefront per row of S [rows][ld] (queries from row0; `cols` prototypes of one segment): s = S o inv_phi, lse, the per-row loss, and S overwritten by
// d loss / d S = (softmax(s) - onehot(y)) o inv_phi * inv, zeros in the pad columns
__global__ void __launch_bounds__(256) pn_row_k(float* __restrict__ S, int rows, int cols, int ld, int row0, const float* __restrict__ ip,
                                                const int32_t* __restrict__ labels, float inv, float* __restrict__ lse, float* __restrict__ rl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= rows) return;
  float* s = S + (int64_t)r * ld;
  float mx = -INFINITY;
  // the score is the ROUNDED product everywhere (__fmul_rn: never contracted into a subtraction), so lse - s_y is exactly zero where the softmax has one term
  for (int j = lane; j < cols; j += 64) mx = fmaxf(mx, mul_rn(s[j], ip[j]));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < cols; j += 64) sum += expf(fmaf(s[j], ip[j], -mx));        // the exponent from the UNROUNDED product: rounding a score at |s| ~ 20 would cost p 1e-6
  sum = wave_sum(sum);
  const float lg = logf(sum), l = mx + lg;
  int y = labels[row0 + r];
  y = y < 0 ? 0 : (y >= cols ? cols - 1 : y);                            // out of range: reported by pn_check_k, never dereferenced
  const float rloss = lg + fmaf(-s[y], ip[y], mx);
  __builtin_amdgcn_wave_barrier();                                      // every lane has read s[y] before lane y % 64 overwrites it
  for (int j = lane; j < ld; j += 64) s[j] = j < cols ? (expf(fmaf(s[j], ip[j], -l)) - (j == y ? 1.f : 0.f)) * ip[j] * inv : 0.f;
  // not l - s_y: l is rounded at lse's magnitude; and the positive's product enters the difference unrounded (the fma), which spares the loss a rounding at |s_y|
  if (lane == 0) { lse[row0 + r] = l; rl[row0 + r] = rloss; }
}

int read_segments(int32_t segs, const int64_t* seg_end, SegTab& tab) {
  tab.segs = segs;
  int64_t prev = 0;
  int first = 0;
  for (int s = 0; s < segs; ++s) {
    const int64_t e = seg_end[s];
    if (e <= prev || e >= (1ll << 31)) return 1;
    const int64_t k = e - prev;
    const int64_t L = (int64_t)SLICE * cdiv64(cdiv64(k, SLICE), MAX_SLICES);
    tab.begin[s] = (int)prev; tab.end[s] = (int)e; tab.rows[s] = (int)L; tab.first[s] = first;
    first += (int)cdiv64(k, L);
    prev = e;
  }
  for (int s = segs; s <= MAX_SEGS; ++s) tab.first[s] = first;
  return 0;
}

}  // namespace

extern "C" size_t ssv_proto_nce_workspace_bytes(int32_t m, int64_t ktot, int32_t d, int32_t segs, int32_t arithmetic) {
  if (!shape_ok(m, ktot, d, segs) || !arith_ok(arithmetic)) return 0;
  return make_plan(m, ktot, d, segs, arithmetic).total();
}

extern "C" int ssv_proto_nce(int32_t m, int32_t d, int32_t segs, const int64_t* seg_end, const float* q, const float* protos, const float* inv_phi,
                             const int32_t* labels, float* loss, float* lse, float* dq, int32_t* flag, int32_t arithmetic, void* ws, size_t ws_bytes,
                             void* stream) {
  SSV_REQUIRE(m >= 1 && m <= MAX_M && segs >= 1 && segs <= MAX_SEGS && d >= 4 && d <= MAX_D && d % 4 == 0,
              "ssv_proto_nce: need 1 <= m <= %d, 1 <= segs <= %d, d %% 4 == 0, 4 <= d <= %d (got m=%d segs=%d d=%d)", MAX_M, MAX_SEGS, MAX_D, m, segs, d);
  SSV_REQUIRE(arith_ok(arithmetic), "ssv_proto_nce: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE(seg_end && q && protos && inv_phi && labels && loss && lse && dq && flag && ws, "ssv_proto_nce: null pointer");
  SegTab tab = {};
  SSV_REQUIRE(read_segments(segs, seg_end, tab) == 0, "ssv_proto_nce: seg_end must be strictly increasing from at least 1 and stay below 2^31");
  const int64_t ktot = tab.end[segs - 1];
  SSV_REQUIRE((((uintptr_t)q | (uintptr_t)protos | (uintptr_t)inv_phi | (uintptr_t)labels | (uintptr_t)loss | (uintptr_t)lse | (uintptr_t)dq | (uintptr_t)flag |
                (uintptr_t)ws) & 15) == 0, "ssv_proto_nce: pointers must be 16-byte aligned");
  const void* in[5] = {q, protos, inv_phi, labels, ws};
  const void* out[4] = {loss, lse, dq, flag};
  SSV_REQUIRE(no_alias(out, 4, in, 5), "ssv_proto_nce: loss, lse, dq and flag alias neither each other nor an input or the workspace");
  const Plan p = make_plan(m, ktot, d, segs, arithmetic);
  SSV_REQUIRE(ws_bytes >= p.total(), "ssv_proto_nce: workspace %zu < %zu bytes", ws_bytes, p.total());
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  float* spos = (float*)w; w += p.spos_bytes;
  float* rl = (float*)w; w += p.rl_bytes;
  const float inv = 1.f / ((float)segs * (float)m);
  {
    ProfScope ps(SSV_PROF_LOSS, s);
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) SSV_FAIL(SSV_ERR_LAUNCH, "ssv_proto_nce: hipMemsetAsync failed");
    const int64_t n = ktot > (int64_t)segs * m ? ktot : (int64_t)segs * m;
    hipLaunchKernelGGL(pn_check_k, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, tab, m, ktot, inv_phi, labels, flag);
    SSV_CHECK_LAUNCH("pn_check_k");
  }
  if (p.fused) {
    ProfScope ps(SSV_PROF_LOSS, s);
    float* pm = (float*)w; w += p.pm_bytes;
    float* pl = (float*)w; w += p.pm_bytes;
    float* pacc = (float*)w; w += p.pacc_bytes;
    u32x4* planes = (u32x4*)w;
    const int NS = d / 16, nsl = tab.first[segs];
    hipLaunchKernelGGL(pn_prep_k, dim3((unsigned)cdiv(NS * p.T, 4)), dim3(256), 0, s, d, m, p.T, NS, q, planes);
    SSV_CHECK_LAUNCH("pn_prep_k");
    SSV_FUSED_LADDER(pn_fused_k, p, dim3((unsigned)nsl, (unsigned)cdiv(p.T, p.KT)), s, protos, inv_phi, labels, tab, m, p.T, p.mpad, (const u32x4*)planes, pm, pl,
                     pacc, spos);
    SSV_CHECK_LAUNCH("pn_fused_k");
    hipLaunchKernelGGL(pn_fold_k, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, s, tab, m, d, p.mpad, (const float*)pm, (const float*)pl, (const float*)pacc,
                       (const float*)spos, protos, inv_phi, labels, inv, lse, rl, dq);
    SSV_CHECK_LAUNCH("pn_fold_k");
  } else {
    float* S = (float*)w; w += p.s_bytes;
    float* cpad = (float*)w;
    for (int sg = 0; sg < segs; ++sg) {
      const int64_t k = tab.end[sg] - tab.begin[sg], kp = (k + 15) / 16 * 16;
      {
        ProfScope ps(SSV_PROF_LOSS, s);
        hipLaunchKernelGGL(pn_pad_k, dim3((unsigned)cdiv64(kp * (d / 4), 256)), dim3(256), 0, s, k, kp, d / 4, (const f32x4*)(protos + (int64_t)tab.begin[sg] * d),
                           (f32x4*)cpad);
        SSV_CHECK_LAUNCH("pn_pad_k");
      }
      for (int r0 = 0; r0 < m; r0 += p.cr) {
        const int rows = m - r0 < p.cr ? m - r0 : p.cr;
        ssv_conv_desc cd = gemm_conv_desc(rows, d, (int)kp, SSV_ARITH_F32_MFMA);
        if (int rc = ssv_conv2d_fwd(&cd, q + (int64_t)r0 * d, cpad, nullptr, nullptr, S, stream)) return rc;      // S[rows, kp] = Q[r0 : r0 + rows] C_seg^T
        {
          ProfScope ps(SSV_PROF_LOSS, s);
          hipLaunchKernelGGL(pn_row_k, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, S, rows, (int)k, (int)kp, r0, inv_phi + tab.begin[sg],
                             labels + (int64_t)sg * m, inv, lse + (int64_t)sg * m, rl + (int64_t)sg * m);
          SSV_CHECK_LAUNCH("pn_row_k");
        }
        float* dx = dq + (int64_t)r0 * d;
        if (int rc = ssv_conv2d_dgrad(&cd, S, cpad, sg ? dx : nullptr, dx, stream)) return rc;                    // dq (+)= dS C_seg, the segments in ascending order
      }
    }
  }
  ProfScope ps(SSV_PROF_LOSS, s);
  hipLaunchKernelGGL(pn_loss_k, dim3(1), dim3(256), 0, s, segs * m, (const float*)rl, inv, loss);
  SSV_CHECK_LAUNCH("pn_loss_k");
  return SSV_OK;
}
