// The nearest-neighbour lookup of NNCLR (Dwibedi et al., ICCV 2021): for every query the bank row with the largest inner product, and that row (scaled).
// The contract is in include/ssv_hip.h (ssv_nn_lookup); the order rule everywhere below is "the best starts at (-inf, 0), only a strictly greater score
// replaces it, candidates are folded in ascending j" - wherever two candidates meet out of order (the two halves of a wave, the lanes of the row kernels) the
// library's arg-max step (value descending, the LOWER index on equal values) gives the same winner, and a part without a winner carries (-inf, 0).
//
//   * SSV_ARITH_BF16X3, d % 32 == 0, d <= SSV_NN_LOOKUP_FUSED_MAX_D: FUSED (nn_fused_k).  S = Q B^T never reaches memory.  The BANK is streamed in fp32 and
//     split into the three bf16 planes in registers (csrc/split_bf16.h: split8), the way kmeans_fused_k streams x - no per-call re-split of a 100 MB queue - but as
//     the A operand of v_mfma_f32_32x32x16_bf16 (lane l: bank row l & 31 of the tile, d = 16 s + 8 (l >> 5) + 0..7).  The QUERIES (m <= 8192: at most a few MB,
//     L2-resident) are split once per call into fragment order (nn_prep_k: prep_planes of csrc/bank_softmax.h, kmeans_prep_k's layout) and are the B operand, so a LANE owns a QUERY: element r of the
//     32 x 32 accumulator in lane (c, h) is the score of query c against bank row acc32_row(r, h) of the tile, and the arg-max over the bank is one compare-select
//     per accumulator element INSIDE the lane - no column-wise reduction over the tile.  A workgroup owns one slice of the bank (SSV_NN_LOOKUP_SLICE rows; a
//     multiple of it above 2^21 rows) and one block of KT <= 8 query tiles (256 queries): its four waves take the four quarters of the slice, 32 rows at a time, and
//     fold them in ascending order through LDS.  Grid: slices x query blocks - 192 x 4 workgroups at 1024 queries against 98,304 rows.  Per-slice (score, index)
//     partials go to the workspace; nn_fold_k folds them in ascending slice order and gathers the row.
//   * SSV_ARITH_F32_MFMA, or a width the fused kernel does not take: S by chunks of queries and parts of the bank on the implicit-GEMM kernel (fp32 MFMA) into the
//     workspace, one wavefront per row (nn_rowarg_k, the pattern of kmeans_rowarg_k) which folds the part into the running best; then nn_fold_k.
//   Every bank row runs ONE instruction sequence on either route whatever its position (a row of the A operand / a column of the GEMM), so bit-identical rows score
//   bit-identically and a duplicate never beats its first copy.  Rows behind n are never read: the fused kernel repeats row n - 1 and masks by index.
#include "bank_softmax.h"

namespace {

using banksm::arith_ok;

constexpr int SLICE = SSV_NN_LOOKUP_SLICE, MAX_SLICES = SSV_NN_LOOKUP_MAX_SLICES, FUSED_MAX_D = SSV_NN_LOOKUP_FUSED_MAX_D;
constexpr int MAX_M = SSV_NN_LOOKUP_MAX_M, MAX_D = SSV_KNN_MAX_D;
constexpr int CHUNK_ROWS = 1024;                                         // query rows of one chunk of S (unfused).  This file's own rule, not banksm::chunk_rows: the bank is cut into parts here, so there is no element cap
constexpr int64_t PART_ELEMS = 1ll << 26, MAX_PART_COLS = 65536;          // one part of the bank on the unfused route: the partition of ssv_knn_search

struct Plan {
  bool fused;
  int T, S4, mpad;            // fused: tiles of 32 queries, slabs of 16 columns (a multiple of 4), queries with the pad of the last tile
  int64_t L, P;               // fused: rows of one slice, slices.  unfused: P = 1 (the running best)
  int cr; int64_t pc;         // unfused: query rows of a chunk, bank rows of a part
  size_t part_bytes, planes_bytes, s_bytes;
  size_t total() const { return 2 * part_bytes + planes_bytes + s_bytes; }
};

bool shape_ok(int32_t m, int64_t n, int32_t d) { return m >= 1 && m <= MAX_M && n >= 1 && n < (1ll << 31) && d >= 4 && d <= MAX_D && d % 4 == 0; }

Plan make_plan(int32_t m, int64_t n, int32_t d, int32_t arithmetic) {
  Plan p = {};
  p.fused = arithmetic == SSV_ARITH_BF16X3 && d % 32 == 0 && d <= FUSED_MAX_D;
  if (p.fused) {
    p.T = cdiv(m, 32); p.S4 = cdiv(d, 64) * 4; p.mpad = p.T * 32;
    p.L = SLICE * cdiv64(cdiv64(n, SLICE), MAX_SLICES);
    p.P = cdiv64(n, p.L);
    p.planes_bytes = (size_t)3 * p.S4 * p.T * 1024;
  } else {
    p.mpad = m; p.P = 1;
    int64_t cap = PART_ELEMS / d;
    if (cap > MAX_PART_COLS) cap = MAX_PART_COLS;
    p.pc = cdiv64(n, cdiv64(n, cap));
    p.cr = m < CHUNK_ROWS ? m : CHUNK_ROWS;
    p.s_bytes = up256((size_t)p.cr * p.pc * 4);
  }
  p.part_bytes = up256((size_t)p.P * p.mpad * 4);
  return p;
}

// the queries' three planes in fragment order with S4 slabs (banksm::prep_planes): S4 is a multiple of 4, so the slabs behind d are there and hold zeros
__global__ void __launch_bounds__(256) nn_prep_k(int d, int m, int T, int S4, const float* __restrict__ q, u32x4* __restrict__ planes) {
  banksm::prep_planes<true>(d, m, T, S4, q, planes);
}

template <int KT>
__global__ void __launch_bounds__(256, KT >= 4 ? 1 : 2)
nn_fused_k(const float* __restrict__ bank, int n, int d, int T, int S4, int L, int mpad, const u32x4* __restrict__ planes, float* __restrict__ pscore,
           int32_t* __restrict__ pidx) {
  __shared__ float sb[4][KT * 32];
  __shared__ int si[4][KT * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int tb = blockIdx.y * KT;
  const int nch = S4 >> 2;
  const int64_t nfrag = (int64_t)S4 * T;
  int tt[KT];                                                           // tiles behind the last repeat it (their results are not written)
#pragma unroll
  for (int t = 0; t < KT; ++t) tt[t] = min(tb + t, T - 1);
  auto frag = [&](int s, int t, int q) { return __builtin_bit_cast(bf16x8, planes[(q * nfrag + (int64_t)s * T + tt[t]) * 64 + lane]); };
  float best[KT];
  int bi[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) { best[t] = -INFINITY; bi[t] = 0; }
  // the wave's quarter of the slice, 32 bank rows at a time (bounds are uniform over the wave: the matrix instructions run with all lanes)
  const int64_t q0 = (int64_t)blockIdx.x * L + (int64_t)wave * (L >> 2);
  const int64_t q1 = q0 + (L >> 2) < (int64_t)n ? q0 + (L >> 2) : (int64_t)n;
  for (int64_t r0 = q0; r0 < q1; r0 += 32) {
    const int64_t brow = r0 + c < (int64_t)n ? r0 + c : (int64_t)n - 1;   // rows behind the end repeat the last one and are masked by index below
    const float* bp = bank + brow * d + 8 * half;
    auto load_b = [&](int ch, f32x4 (&r)[8]) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int col = 64 * ch + 16 * (i >> 1) + 8 * half + 4 * (i & 1);            // d % 4 == 0: a float4 is inside the row or behind it
        r[i] = col < d ? *(const f32x4*)(bp + 64 * ch + 16 * (i >> 1) + 4 * (i & 1)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    };
    f32x16 acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    constexpr int NB = 4, STEPS = 4 * KT;                               // a ring of query fragments, three (slab, tile) steps ahead of the products
    bf16x8 kf[NB][3];
#pragma unroll
    for (int st = 0; st < NB - 1; ++st)
#pragma unroll
      for (int q = 0; q < 3; ++q) kf[st][q] = frag(st / KT, st % KT, q);
    f32x4 xr[8];
    load_b(0, xr);
    for (int ch = 0; ch < nch; ++ch) {
      f32x4 xn[8];
      const int chn = min(ch + 1, nch - 1);
      load_b(chn, xn);                                                  // the last chunk is loaded twice rather than branching around the prefetch
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) {
        bf16x8 xb[3];
        splitbf::split8(xr[2 * sl], xr[2 * sl + 1], xb);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          const int st = sl * KT + t, nx = st + NB - 1;                  // compile-time after unrolling
#pragma unroll
          for (int q = 0; q < 3; ++q)
            kf[nx % NB][q] = nx < STEPS ? frag(4 * ch + nx / KT, nx % KT, q) : frag(4 * chn + (nx - STEPS) / KT, (nx - STEPS) % KT, q);
          splitbf::mma6_32(acc[t], xb, kf[st % NB]);                     // A: the bank rows (accumulator rows), B: the queries (one per lane)
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[i] = xn[i];
    }
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = r0 + splitbf::acc32_row(r, half);
        const float sc = acc[t][r];
        const bool up = sc > best[t] && j < (int64_t)n;                  // strict: within a lane the indices ascend, the first maximum stays (NaN never enters)
        best[t] = up ? sc : best[t];
        bi[t] = up ? (int)j : bi[t];
      }
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    SSV_ARGMAX_FIRST_STEP(best[t], bi[t], 32);                           // the query's other half of every tile's rows
    if (half == 0) { sb[wave][t * 32 + c] = best[t]; si[wave][t * 32 + c] = bi[t]; }
  }
  __syncthreads();
  const int u = threadIdx.x;
  if (u < KT * 32 && tb + (u >> 5) < T) {
    float v = sb[0][u];
    int vi = si[0][u];
#pragma unroll
    for (int w = 1; w < 4; ++w) {                                        // the quarters ascend: strict >
      const bool up = sb[w][u] > v;
      v = up ? sb[w][u] : v;
      vi = up ? si[w][u] : vi;
    }
    const int64_t o = (int64_t)blockIdx.x * mpad + 32 * tb + u;
    pscore[o] = v;
    pidx[o] = vi;
  }
}

// the unfused route: one wavefront per row of S [rows][cols] (queries from row0, bank rows from c0) folds the part into the running best of its query
__global__ void __launch_bounds__(256) nn_rowarg_k(const float* __restrict__ S, int rows, int cols, int row0, int c0, float* __restrict__ pscore,
                                                   int32_t* __restrict__ pidx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= rows) return;
  const float* s = S + (int64_t)r * cols;
  float best = -INFINITY;
  int bi = 0;
  for (int j = lane; j < cols; j += 64) {
    const float sc = s[j];
    if (sc > best) { best = sc; bi = c0 + j; }
  }
  SSV_WAVE_ARGMAX_FIRST(best, bi);
  if (lane == 0) {
    if (c0 > 0) {                                                        // the parts ascend: strict >
      const float pv = pscore[row0 + r];
      if (!(best > pv)) { best = pv; bi = pidx[row0 + r]; }
    }
    pscore[row0 + r] = best;
    pidx[row0 + r] = bi;
  }
}

// one wavefront per query: the P partials in ascending order, then idx, sim and the scaled row
__global__ void __launch_bounds__(256) nn_fold_k(int m, int d, int P, int mpad, const float* __restrict__ pscore, const int32_t* __restrict__ pidx,
                                                 const float* __restrict__ bank, float out_scale, float* __restrict__ nn, int32_t* __restrict__ idx,
                                                 float* __restrict__ sim) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= m) return;
  float best = -INFINITY;
  int bi = 0;
  for (int p = lane; p < P; p += 64) {
    const float sc = pscore[(int64_t)p * mpad + i];
    if (sc > best) { best = sc; bi = pidx[(int64_t)p * mpad + i]; }
  }
  SSV_WAVE_ARGMAX_FIRST(best, bi);
  if (lane == 0) { idx[i] = bi; sim[i] = best; }
  if (nn) {
    const float* b = bank + (int64_t)bi * d;
    for (int e = lane * 4; e < d; e += 256) {
      const f32x4 v = *(const f32x4*)(b + e);
      *(f32x4*)(nn + (int64_t)i * d + e) = f32x4{out_scale * v[0], out_scale * v[1], out_scale * v[2], out_scale * v[3]};
    }
  }
}

}  // namespace

extern "C" size_t ssv_nn_lookup_workspace_bytes(int32_t m, int64_t n, int32_t d, int32_t arithmetic) {
  if (!shape_ok(m, n, d) || !arith_ok(arithmetic)) return 0;
  return make_plan(m, n, d, arithmetic).total();
}

extern "C" int ssv_nn_lookup(int32_t m, int64_t n, int32_t d, const float* queries, const float* bank, float out_scale, float* nn, int32_t* idx, float* sim,
                             int32_t arithmetic, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(m, n, d), "ssv_nn_lookup: need 1 <= m <= %d, 1 <= n < 2^31, d %% 4 == 0, 4 <= d <= %d (got m=%d n=%lld d=%d)", MAX_M, MAX_D, m, (long long)n, d);
  SSV_REQUIRE(arith_ok(arithmetic), "ssv_nn_lookup: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE(isfinite(out_scale), "ssv_nn_lookup: out_scale must be finite (got %g)", (double)out_scale);
  SSV_REQUIRE(queries && bank && idx && sim && ws, "ssv_nn_lookup: null pointer (only nn may be NULL)");
  SSV_REQUIRE((((uintptr_t)queries | (uintptr_t)bank | (uintptr_t)nn | (uintptr_t)idx | (uintptr_t)sim | (uintptr_t)ws) & 15) == 0, "ssv_nn_lookup: pointers must be 16-byte aligned");
  const void* in[3] = {queries, bank, ws};
  const void* out[3] = {idx, sim, nn};
  SSV_REQUIRE(no_alias(out, 3, in, 3), "ssv_nn_lookup: nn, idx and sim alias neither each other nor an input or the workspace");
  const Plan p = make_plan(m, n, d, arithmetic);
  SSV_REQUIRE(ws_bytes >= p.total(), "ssv_nn_lookup: workspace %zu < %zu bytes", ws_bytes, p.total());
  hipStream_t s = (hipStream_t)stream;
  float* pscore = (float*)ws;
  int32_t* pidx = (int32_t*)((char*)ws + p.part_bytes);
  void* rest = (char*)ws + 2 * p.part_bytes;
  if (p.fused) {
    ProfScope ps(SSV_PROF_MISC, s);
    u32x4* planes = (u32x4*)rest;
    hipLaunchKernelGGL(nn_prep_k, dim3((unsigned)cdiv(p.S4 * p.T, 4)), dim3(256), 0, s, d, m, p.T, p.S4, queries, planes);
    SSV_CHECK_LAUNCH("nn_prep_k");
#define SSV_NN(KT) hipLaunchKernelGGL(nn_fused_k<KT>, dim3((unsigned)p.P, (unsigned)cdiv(p.T, KT)), dim3(256), 0, s, bank, (int)n, d, p.T, p.S4, (int)p.L, p.mpad, \
                                      (const u32x4*)planes, pscore, pidx)
    if (p.T == 1) SSV_NN(1); else if (p.T == 2) SSV_NN(2); else if (p.T <= 4) SSV_NN(4); else SSV_NN(8);
#undef SSV_NN
    SSV_CHECK_LAUNCH("nn_fused_k");
  } else {
    float* S = (float*)rest;
    for (int64_t c0 = 0; c0 < n; c0 += p.pc) {
      const int cols = (int)(n - c0 < p.pc ? n - c0 : p.pc);
      for (int r0 = 0; r0 < m; r0 += p.cr) {
        const int rows = m - r0 < p.cr ? m - r0 : p.cr;
        ssv_conv_desc cd = gemm_conv_desc(rows, d, cols, SSV_ARITH_F32_MFMA);
        if (int rc = ssv_conv2d_fwd(&cd, queries + (int64_t)r0 * d, bank + c0 * d, nullptr, nullptr, S, stream)) return rc;   // S[rows, cols] = Q[r0 : r0 + rows] B[c0 : c0 + cols]^T
        ProfScope ps(SSV_PROF_MISC, s);
        hipLaunchKernelGGL(nn_rowarg_k, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, (const float*)S, rows, cols, r0, (int)c0, pscore, pidx);
        SSV_CHECK_LAUNCH("nn_rowarg_k");
      }
    }
  }
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(nn_fold_k, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, s, m, d, (int)p.P, p.mpad, (const float*)pscore, (const int32_t*)pidx, bank, out_scale, nn, idx,
                     sim);
  SSV_CHECK_LAUNCH("nn_fold_k");
  return SSV_OK;
}
