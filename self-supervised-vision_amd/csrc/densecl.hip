// DenseCL (Wang, Zhang, Shen, Kong, Li, CVPR 2021): the two kernels of its dense term.  The contracts are in include/ssv_hip.h (ssv_dense_match, ssv_queue_nce).
//
// ssv_dense_match: per image the s x s scores of the cells of view 1 against the cells of view 2, reduced to an arg-max per cell of view 1.  One workgroup per
//   (image, tile of 32 cells of view 1); its four waves take the tiles of 32 cells of view 2 (wave w: tiles w and w + 4).  Both maps are read in fp32 straight
//   into fragment order (a lane owns a row of its operand and 8 consecutive channels of a 16-wide slab) - view 2 is the A operand, view 1 the B operand, so a
//   LANE owns a cell of view 1 and the arg-max over a tile is compare-select inside the lane.  The squared norms of both operands are summed in fp32 from the same
//   registers.  SSV_ARITH_BF16X3: the six-product accumulation of split_bf16.h on v_mfma_f32_32x32x16_bf16; SSV_ARITH_F32_MFMA: v_mfma_f32_32x32x2_f32 on the same
//   registers (instruction e contracts channels e and 8 + e of the slab).  The score tile lives in the accumulators and is never written.
//
// ssv_queue_nce: InfoNCE of every query against a queue, with one positive per query gathered from another matrix.  The queue carries no gradient, so the loss
//   and d loss / d q are one pass of the shape of a flash-attention forward.
//   * SSV_ARITH_BF16X3, d % 32 == 0, d <= SSV_QUEUE_NCE_FUSED_MAX_D: FUSED (qn_fused_k): the pass of csrc/bank_softmax_pass.h (described in csrc/protonce.hip) with the source Range, one temperature - bank rows
//     streamed in fp32 and split in registers as the A operand, the queries split once per call into fragment order (qn_prep_k) as the B operand, the second
//     product out^T += V^T P^T under the online rescale with the tile of bank rows read back transposed from LDS in the order in which P lies in the accumulators.
//     A workgroup owns one slice of the queue (L rows, a multiple of SSV_QUEUE_NCE_SLICE) and one block of KT query tiles; its four waves take the four quarters
//     of the slice and leave (max, sum, acc[d]) in the workspace.  The number of slices is a pure function of the shape (make_plan): enough workgroups for
//     SSV_QUEUE_NCE_TARGET_WGS, never more than SSV_QUEUE_NCE_MAX_SLICES - at DenseCL's shapes m / 32 query tiles fill the machine and the queue is ONE slice.
//     qn_fold_k merges the partials in ascending order and then the POSITIVE as one more partial: its score is a d-long fp32 dot product of the query with
//     keys[pos[i]], its row enters the accumulator with its probability.  It subtracts the positive's row and writes lse and dq; qn_loss_k sums the rows' losses.
//   * SSV_ARITH_F32_MFMA, or another width: UNFUSED, per chunk of queries: S on ssv_conv2d_fwd against a copy of the queue padded with zero rows to a multiple
//     of 16 (the data-gradient GEMM contracts whole 16-row groups), one wavefront per row reduces it together with the positive and overwrites S with
//     d loss / d S (qn_row_k, which also leaves the positive's share of dq), ssv_conv2d_dgrad adds dS bank.
//   Numerics of both routes (protonce.hip's): the maximum and lse take the ROUNDED score (one fp32 multiply by inv_temp), the exponents take the unrounded
//   product through an fma, the row loss is log(sum) + (max - s+).  The positive's d products are summed in double and rounded to the fp32 dot product once;
//   a row's sum, its logarithm, its loss (with s+ from the unrounded dot product) and the mean over the rows are carried in double, so the loss takes one
//   fp32 rounding at the end - with one query the loss is one row's, and fp32 steps there would each cost it half an ulp.
// No floating-point atomics anywhere; every workspace value that is read was written by the same call.
#include "bank_softmax.h"

namespace {

using banksm::arith_ok;
using banksm::mul_rn;

constexpr int MATCH_MAX_S = SSV_DENSE_MATCH_MAX_S, MATCH_MAX_C = SSV_DENSE_MATCH_MAX_C;
constexpr int SLICE = SSV_QUEUE_NCE_SLICE, MAX_SLICES = SSV_QUEUE_NCE_MAX_SLICES, FUSED_MAX_D = SSV_QUEUE_NCE_FUSED_MAX_D, TARGET_WGS = SSV_QUEUE_NCE_TARGET_WGS;
constexpr int MAX_M = SSV_QUEUE_NCE_MAX_M, MAX_D = SSV_KNN_MAX_D;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- ssv_dense_match ---------------------------------------------------------------------------------------------------------------------------------------------
// candidates are (score, dot, clamped norm, j): the higher score wins, equal scores go to the lower j
template <int NT, bool BF16>
__global__ void __launch_bounds__(256)
dm_match_k(int s, int c, int qtiles, const float* __restrict__ f1, const float* __restrict__ f2, float eps, int32_t* __restrict__ idx, float* __restrict__ sim) {
  __shared__ float w_s[4][32], w_d[4][32], w_n[4][32];
  __shared__ int w_j[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cc = lane & 31, half = lane >> 5;
  const int64_t n = blockIdx.x / qtiles;
  const int qt = blockIdx.x % qtiles;
  const float* a1 = f1 + n * (int64_t)s * c;
  const float* a2 = f2 + n * (int64_t)s * c;
  const int qi = min(32 * qt + cc, s - 1);                             // cells behind the map repeat its last one (their results are not written)
  const float* qp = a1 + (int64_t)qi * c;
  const float* kp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) kp[t] = a2 + (int64_t)min(32 * (wave + 4 * t) + cc, s - 1) * c;      // likewise, masked by index below
  f32x16 acc[NT];
  float kn2[NT], qn2 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    kn2[t] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  }
  const bool work = 32 * wave < s;                                      // uniform over the wave: a wave without a tile of view 2 skips the products
  if (work) {
    for (int col = 8 * half; col < c + 8 * half; col += 16) {           // both halves run the same number of slabs (the matrix instructions need all lanes)
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 qa = col < c ? *(const f32x4*)(qp + col) : z, qb = col + 4 < c ? *(const f32x4*)(qp + col + 4) : z;
      qn2 += qa[0] * qa[0] + qa[1] * qa[1] + qa[2] * qa[2] + qa[3] * qa[3] + qb[0] * qb[0] + qb[1] * qb[1] + qb[2] * qb[2] + qb[3] * qb[3];
      bf16x8 qf[3];
      if constexpr (BF16) splitbf::split8(qa, qb, qf);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 ka = col < c ? *(const f32x4*)(kp[t] + col) : z, kb = col + 4 < c ? *(const f32x4*)(kp[t] + col + 4) : z;
        kn2[t] += ka[0] * ka[0] + ka[1] * ka[1] + ka[2] * ka[2] + ka[3] * ka[3] + kb[0] * kb[0] + kb[1] * kb[1] + kb[2] * kb[2] + kb[3] * kb[3];
        if constexpr (BF16) {
          bf16x8 kf[3];
          splitbf::split8(ka, kb, kf);
          splitbf::mma6_32(acc[t], kf, qf);                             // A: the cells of view 2 (accumulator rows), B: the cells of view 1 (one per lane)
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], qa[e], acc[t], 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[e], qb[e], acc[t], 0, 0, 0);
        }
      }
    }
  }
  qn2 += __shfl_xor(qn2, 32, 64);
  float bs = -INFINITY, bd = 0.f, bn = 1.f;
  int bj = 0x7fffffff;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float kn = sqrtf(kn2[t] + __shfl_xor(kn2[t], 32, 64));        // |f2_j| of the cell this lane loaded: lanes r and r + 32 hold cell r of the tile
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = splitbf::acc32_row(r, half), j = 32 * (wave + 4 * t) + row;
      const float nj = fmaxf(__shfl(kn, row, 64), eps);
      if (j < s) {
        const float sc = acc[t][r] / nj;
        const bool take = sc > bs || (sc == bs && j < bj);
        bs = take ? sc : bs; bd = take ? acc[t][r] : bd; bn = take ? nj : bn; bj = take ? j : bj;
      }
    }
  }
  {                                                                     // the other half of the query's column
    const float os = __shfl_xor(bs, 32, 64), od = __shfl_xor(bd, 32, 64), on = __shfl_xor(bn, 32, 64);
    const int oj = __shfl_xor(bj, 32, 64);
    const bool take = os > bs || (os == bs && oj < bj);
    bs = take ? os : bs; bd = take ? od : bd; bn = take ? on : bn; bj = take ? oj : bj;
  }
  if (half == 0) { w_s[wave][cc] = bs; w_d[wave][cc] = bd; w_n[wave][cc] = bn; w_j[wave][cc] = bj; }
  __syncthreads();
  if (wave == 0 && half == 0 && 32 * qt + cc < s) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float os = w_s[w][cc];
      const int oj = w_j[w][cc];
      const bool take = os > bs || (os == bs && oj < bj);
      bs = take ? os : bs; bd = take ? w_d[w][cc] : bd; bn = take ? w_n[w][cc] : bn; bj = take ? oj : bj;
    }
    const int64_t o = n * s + 32 * qt + cc;
    if (bj >= s) { bj = 0; bd = NAN; }                                  // every score of the cell is NaN: cell 0, and sim says so
    idx[o] = (int32_t)(n * s + bj);
    sim[o] = bd / (fmaxf(sqrtf(qn2), eps) * bn);
  }
}

// ---- ssv_queue_nce: the plan -----------------------------------------------------------------------------------------------------------------------------------
struct Plan : banksm::FusedPlan {
  bool fused;
  int nsl; int64_t L;                                 // fused: slices, rows of one slice
  int cr; int64_t kp;                                 // unfused: query rows of a chunk, rows of the queue rounded up to 16
  size_t rl_bytes, s_bytes, bpad_bytes;
  size_t total() const { return rl_bytes + 2 * pm_bytes + pacc_bytes + planes_bytes + s_bytes + bpad_bytes; }
};

bool shape_ok(int32_t m, int64_t K, int32_t d) {
  return m >= 1 && m <= MAX_M && K >= 1 && K < (1ll << 31) && d >= 4 && d <= MAX_D && d % 4 == 0;
}
bool is_fused(int32_t d, int32_t arithmetic) { return arithmetic == SSV_ARITH_BF16X3 && d % 32 == 0 && d <= FUSED_MAX_D; }
// the GEMM route describes the padded queue to the convolution entry points with 32-bit sizes
bool route_ok(int64_t K, int32_t d, int32_t arithmetic) { return is_fused(d, arithmetic) || K <= (1ll << 31) - 16; }

Plan make_plan(int32_t m, int64_t K, int32_t d, int32_t arithmetic) {
  Plan p = {};
  p.fused = is_fused(d, arithmetic);
  p.rl_bytes = up256((size_t)m * 8);                  // the rows' losses in double: the mean is rounded to fp32 once
  if (p.fused) {
    banksm::plan_tiles(p, m, d);
    const int blocks = cdiv(p.T, p.KT);
    int64_t want = cdiv(TARGET_WGS, blocks);            // slices only as far as a small m needs them
    if (want > MAX_SLICES) want = MAX_SLICES;
    const int64_t units = cdiv64(K, SLICE);
    if (want > units) want = units;
    p.L = (int64_t)SLICE * cdiv64(units, want);
    p.nsl = (int)cdiv64(K, p.L);
    banksm::plan_bytes(p, p.nsl, d);
  } else {
    p.mpad = m;
    p.kp = (K + 15) / 16 * 16;
    p.cr = banksm::chunk_rows(p.kp, m);
    p.s_bytes = up256((size_t)p.cr * p.kp * 4);
    p.bpad_bytes = up256((size_t)p.kp * d * 4);
  }
  return p;
}

// the per-row losses rl [n] in a fixed order: thread t takes t, t + 256, ..., then the fixed tree; in double, so the mean takes ONE fp32 rounding
__global__ void __launch_bounds__(256) qn_loss_k(int n, const double* __restrict__ rl, float* __restrict__ loss) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += rl[i];
  sm[threadIdx.x] = a;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) loss[0] = (float)(sm[0] / (double)n);
}

// ---- fused -------------------------------------------------------------------------------------------------------------------------------------------------------
// the queries' three planes in fragment order with d / 16 slabs (banksm::prep_planes); rows behind m are zeros
__global__ void __launch_bounds__(256) qn_prep_k(int d, int m, int T, int NS, const float* __restrict__ q, u32x4* __restrict__ planes) {
  banksm::prep_planes<false>(d, m, T, NS, q, planes);
}

// the pass of bank_softmax_pass.h over one slice of the queue: rows [0, K), one temperature, the bare rows as V, the positive outside the bank (qn_fold_k adds it)
template <int DT, int KT>
__global__ void __launch_bounds__(256, 1)
qn_fused_k(const float* __restrict__ bank, int64_t K, int64_t L, float inv_temp, int T, int mpad, int blocks, const u32x4* __restrict__ planes,
           float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ pacc) {
  constexpr int D = 32 * DT;
  __shared__ float vt[4][32 * D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int sl = blockIdx.x / blocks, tb = (blockIdx.x % blocks) * KT;
  const int64_t end = K;
  const auto slice0 = [&] { return (int64_t)sl * L; };                                     // evaluated where the pass needs it
  using SRC = banksm::Range;
  const SRC src = {nullptr, nullptr, nullptr, 0, 0, 0, inv_temp};
#include "bank_softmax_pass.h"
}

// one wavefront per query: the partials in ascending order, then the positive as one more partial, the positive's row off
__global__ void __launch_bounds__(256) qn_fold_k(int m, int d, int mpad, int parts, int64_t mk, const float* __restrict__ pm, const float* __restrict__ pl,
                                                 const float* __restrict__ pacc, const float* __restrict__ q, const float* __restrict__ keys,
                                                 const int32_t* __restrict__ pos, float inv_temp, float gscale, float* __restrict__ lse, double* __restrict__ rl,
                                                 float* __restrict__ dq, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= m) return;
  constexpr int NE = FUSED_MAX_D / 64;                                  // gscale = inv_temp / m: V is the unscaled bank, so the temperature enters dq here
  int64_t y = pos[i];
  if (y < 0 || y >= mk) {                                               // reported, never dereferenced
    if (lane == 0) atomicOr(flag, 1);
    y = y < 0 ? 0 : mk - 1;
  }
  float kpos[NE];
  double dotd = 0.0;                                                    // the d products are exact in double: the fp32 dot product below is rounded ONCE
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    kpos[k] = lane + 64 * k < d ? keys[y * d + lane + 64 * k] : 0.f;
    if (lane + 64 * k < d) dotd += (double)q[(int64_t)i * d + lane + 64 * k] * (double)kpos[k];
  }
  dotd = wave_sum_d(dotd);
  const float dot = (float)dotd;
  const float sp = mul_rn(dot, inv_temp);                               // the positive's score, rounded like every other
  float M = sp;
  for (int p = 0; p < parts; ++p) M = fmaxf(M, pm[(int64_t)p * mpad + i]);
  double Ld = 0.0;
  float a[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) a[k] = 0.f;
  for (int p = 0; p < parts; ++p) {
    const int64_t o = (int64_t)p * mpad + i;
    const float mp = pm[o];
    const float w = mp == -INFINITY ? 0.f : expf(mp - M);               // a quarter behind the queue's end holds (-inf, 0, 0)
    Ld += (double)pl[o] * (double)w;
#pragma unroll
    for (int k = 0; k < NE; ++k)
      if (lane + 64 * k < d) a[k] += pacc[o * d + lane + 64 * k] * w;
  }
  const float pp = expf(fmaf(dot, inv_temp, -M));                       // the exponent from the unrounded product
  Ld += (double)pp;
  const float Ls = (float)Ld;
#pragma unroll
  for (int k = 0; k < NE; ++k)
    if (lane + 64 * k < d) dq[(int64_t)i * d + lane + 64 * k] = ((a[k] + pp * kpos[k]) / Ls - kpos[k]) * gscale;
  if (lane == 0) {                                                      // log(sum) + (max - s+) in double, s+ from the unrounded dot product: the row's loss takes no rounding here
    const double lg = log(Ld);
    lse[i] = (float)((double)M + lg);
    rl[i] = lg + ((double)M - dotd * (double)inv_temp);
  }
}

// ---- unfused -----------------------------------------------------------------------------------------------------------------------------------------------------
// rows [0, k) of the queue into dst [kp][d], zero rows behind k
__global__ void __launch_bounds__(256) qn_pad_k(int64_t k, int64_t kp, int d4, const f32x4* __restrict__ src, f32x4* __restrict__ dst) {
  banksm::pad_rows(k, kp, d4, src, dst);
}

// one wavefront per row of S [rows][ld] (queries from row0; `cols` queue rows): lse and the row's loss over the positive and the queue, S overwritten by
// d loss / d S = softmax * inv_temp * inv (zeros in the pad columns), and the positive's share (p+ - 1) k+ * inv_temp * inv written to dq
__global__ void __launch_bounds__(256) qn_row_k(float* __restrict__ S, int rows, int cols, int ld, int row0, int d, int64_t mk, const float* __restrict__ q,
                                                const float* __restrict__ keys, const int32_t* __restrict__ pos, float inv_temp, float inv,
                                                float* __restrict__ lse, double* __restrict__ rl, float* __restrict__ dq, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= rows) return;
  const int64_t i = row0 + r;
  float* s = S + (int64_t)r * ld;
  int64_t y = pos[i];
  if (y < 0 || y >= mk) {
    if (lane == 0) atomicOr(flag, 1);
    y = y < 0 ? 0 : mk - 1;
  }
  const float* kr = keys + y * d;
  const float* qr = q + i * d;
  double dotd = 0.0;                                                    // as in qn_fold_k: exact products, one rounding to the fp32 dot product
  for (int k = lane; k < d; k += 64) dotd += (double)qr[k] * (double)kr[k];
  dotd = wave_sum_d(dotd);
  const float dot = (float)dotd;
  const float sp = mul_rn(dot, inv_temp);
  float mx = sp;
  for (int j = lane; j < cols; j += 64) mx = fmaxf(mx, mul_rn(s[j], inv_temp));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < cols; j += 64) sum += expf(fmaf(s[j], inv_temp, -mx));
  const double sumd = wave_sum_d((double)sum) + (double)expf(fmaf(dot, inv_temp, -mx));
  const double lgd = log(sumd);
  const float l = (float)((double)mx + lgd), g = inv_temp * inv;
  for (int j = lane; j < ld; j += 64) s[j] = j < cols ? expf(fmaf(s[j], inv_temp, -l)) * g : 0.f;
  const float cp = (expf(fmaf(dot, inv_temp, -l)) - 1.f) * g;
  for (int k = lane; k < d; k += 64) dq[i * d + k] = cp * kr[k];
  if (lane == 0) { lse[i] = l; rl[i] = lgd + ((double)mx - dotd * (double)inv_temp); }
}

}  // namespace

extern "C" int ssv_dense_match(int32_t b, int32_t s, int32_t c, const float* f1, const float* f2, float eps, int32_t* idx, float* sim, int32_t arithmetic,
                               void* stream) {
  SSV_REQUIRE(b >= 1 && s >= 1 && s <= MATCH_MAX_S && c >= 4 && c <= MATCH_MAX_C && c % 4 == 0 && (int64_t)b * s < (1ll << 31),
              "ssv_dense_match: need b >= 1, 1 <= s <= %d, c %% 4 == 0, 4 <= c <= %d, b * s < 2^31 (got b=%d s=%d c=%d)", MATCH_MAX_S, MATCH_MAX_C, b, s, c);
  SSV_REQUIRE(arith_ok(arithmetic), "ssv_dense_match: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE(eps > 0.f && eps < INFINITY, "ssv_dense_match: eps must be finite and positive");
  SSV_REQUIRE(f1 && f2 && idx && sim, "ssv_dense_match: null pointer");
  SSV_REQUIRE((((uintptr_t)f1 | (uintptr_t)f2 | (uintptr_t)idx | (uintptr_t)sim) & 15) == 0, "ssv_dense_match: pointers must be 16-byte aligned");
  SSV_REQUIRE((const void*)idx != (const void*)sim && (const void*)idx != (const void*)f1 && (const void*)idx != (const void*)f2 &&
              (const void*)sim != (const void*)f1 && (const void*)sim != (const void*)f2, "ssv_dense_match: idx and sim alias neither each other nor an input");
  const int qtiles = cdiv(s, 32);
  SSV_REQUIRE((int64_t)b * qtiles < (1ll << 31), "ssv_dense_match: b * ceil(s / 32) must stay below 2^31");
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, st);
  const dim3 grid((unsigned)(b * qtiles));
#define SSV_DM(NT, BF) hipLaunchKernelGGL((dm_match_k<NT, BF>), grid, dim3(256), 0, st, s, c, qtiles, f1, f2, eps, idx, sim)
  if (arithmetic == SSV_ARITH_BF16X3) { if (s <= 128) SSV_DM(1, true); else SSV_DM(2, true); }
  else { if (s <= 128) SSV_DM(1, false); else SSV_DM(2, false); }
#undef SSV_DM
  SSV_CHECK_LAUNCH("dm_match_k");
  return SSV_OK;
}

extern "C" size_t ssv_queue_nce_workspace_bytes(int32_t m, int64_t K, int32_t d, int32_t arithmetic) {
  if (!shape_ok(m, K, d) || !arith_ok(arithmetic) || !route_ok(K, d, arithmetic)) return 0;
  return make_plan(m, K, d, arithmetic).total();
}

extern "C" int ssv_queue_nce(int32_t m, int32_t d, int64_t K, int64_t mk, const float* q, const float* keys, const int32_t* pos, const float* bank,
                             float inv_temp, float* loss, float* lse, float* dq, int32_t* flag, int32_t arithmetic, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(m, K, d) && mk >= 1 && mk < (1ll << 31),
              "ssv_queue_nce: need 1 <= m <= %d, 1 <= K < 2^31, 1 <= mk < 2^31, d %% 4 == 0, 4 <= d <= %d (got m=%d K=%lld mk=%lld d=%d)", MAX_M, MAX_D, m,
              (long long)K, (long long)mk, d);
  SSV_REQUIRE(arith_ok(arithmetic), "ssv_queue_nce: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE(route_ok(K, d, arithmetic), "ssv_queue_nce: the GEMM route takes at most 2^31 - 16 queue rows (got K=%lld)", (long long)K);
  SSV_REQUIRE(inv_temp > 0.f && inv_temp < INFINITY, "ssv_queue_nce: inv_temp must be finite and positive");
  SSV_REQUIRE(q && keys && pos && bank && loss && lse && dq && flag && ws, "ssv_queue_nce: null pointer");
  SSV_REQUIRE((((uintptr_t)q | (uintptr_t)keys | (uintptr_t)pos | (uintptr_t)bank | (uintptr_t)loss | (uintptr_t)lse | (uintptr_t)dq | (uintptr_t)flag |
                (uintptr_t)ws) & 15) == 0, "ssv_queue_nce: pointers must be 16-byte aligned");
  const void* in[5] = {q, keys, pos, bank, ws};
  const void* out[4] = {loss, lse, dq, flag};
  SSV_REQUIRE(no_alias(out, 4, in, 5), "ssv_queue_nce: loss, lse, dq and flag alias neither each other nor an input or the workspace");
  const Plan p = make_plan(m, K, d, arithmetic);
  SSV_REQUIRE(ws_bytes >= p.total(), "ssv_queue_nce: workspace %zu < %zu bytes", ws_bytes, p.total());
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  double* rl = (double*)w; w += p.rl_bytes;
  const float inv = 1.f / (float)m;
  {
    ProfScope ps(SSV_PROF_LOSS, s);
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) SSV_FAIL(SSV_ERR_LAUNCH, "ssv_queue_nce: hipMemsetAsync failed");
  }
  if (p.fused) {
    ProfScope ps(SSV_PROF_LOSS, s);
    float* pm = (float*)w; w += p.pm_bytes;
    float* pl = (float*)w; w += p.pm_bytes;
    float* pacc = (float*)w; w += p.pacc_bytes;
    u32x4* planes = (u32x4*)w;
    const int NS = d / 16, blocks = cdiv(p.T, p.KT);
    hipLaunchKernelGGL(qn_prep_k, dim3((unsigned)cdiv(NS * p.T, 4)), dim3(256), 0, s, d, m, p.T, NS, q, planes);
    SSV_CHECK_LAUNCH("qn_prep_k");
    SSV_FUSED_LADDER(qn_fused_k, p, dim3((unsigned)(p.nsl * blocks)), s, bank, K, p.L, inv_temp, p.T, p.mpad, blocks, (const u32x4*)planes, pm, pl, pacc);
    SSV_CHECK_LAUNCH("qn_fused_k");
    hipLaunchKernelGGL(qn_fold_k, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, s, m, d, p.mpad, 4 * p.nsl, mk, (const float*)pm, (const float*)pl, (const float*)pacc,
                       q, keys, pos, inv_temp, inv_temp * inv, lse, rl, dq, flag);
    SSV_CHECK_LAUNCH("qn_fold_k");
  } else {
    float* S = (float*)w; w += p.s_bytes;
    float* bpad = (float*)w;
    {
      ProfScope ps(SSV_PROF_LOSS, s);
      hipLaunchKernelGGL(qn_pad_k, dim3((unsigned)cdiv64(p.kp * (d / 4), 256)), dim3(256), 0, s, K, p.kp, d / 4, (const f32x4*)bank, (f32x4*)bpad);
      SSV_CHECK_LAUNCH("qn_pad_k");
    }
    for (int r0 = 0; r0 < m; r0 += p.cr) {
      const int rows = m - r0 < p.cr ? m - r0 : p.cr;
      ssv_conv_desc cd = gemm_conv_desc(rows, d, (int)p.kp, SSV_ARITH_F32_MFMA);
      if (int rc = ssv_conv2d_fwd(&cd, q + (int64_t)r0 * d, bpad, nullptr, nullptr, S, stream)) return rc;      // S[rows, kp] = Q[r0 : r0 + rows] bank^T
      {
        ProfScope ps(SSV_PROF_LOSS, s);
        hipLaunchKernelGGL(qn_row_k, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, S, rows, (int)K, (int)p.kp, r0, d, mk, q, keys, pos, inv_temp, inv, lse, rl, dq,
                           flag);
        SSV_CHECK_LAUNCH("qn_row_k");
      }
      float* dx = dq + (int64_t)r0 * d;
      if (int rc = ssv_conv2d_dgrad(&cd, S, bpad, dx, dx, stream)) return rc;                                   // dq += dS bank
    }
  }
  ProfScope ps(SSV_PROF_LOSS, s);
  hipLaunchKernelGGL(qn_loss_k, dim3(1), dim3(256), 0, s, m, (const double*)rl, loss);
  SSV_CHECK_LAUNCH("qn_loss_k");
  return SSV_OK;
}
