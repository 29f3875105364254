// Lloyd k-means on the GPU and the vote table of the Hungarian-matched cluster accuracy (the metric behind the reference's accuracy table: its README; the reference runs
// faiss.Kmeans over encoder features at models/deep_cluster.py:100-118 and matches clusters to classes at utils/eval_utils.py:23-35, but never joins the two).
//
// Assignment.  label(i) = argmax_j (x_i . c_j - 1/2 |c_j|^2), exact ties to the LOWEST j; dist(i) = |x_i - c_label|^2, summed DIRECTLY over the columns once the
//   label is known (one more read of the row and of one centroid row): |x|^2 - 2 score cancels |x|^2 + |c|^2 against 2 x . c, which left 2^-24 (|x|^2 + |c|^2) of
//   one-sided noise (the clamp at 0) on every row that IS its centroid and a sum chain of d / 2 terms per lane (tests/test_gpu_kmeans_forms.py measured both).
//   * SSV_ARITH_BF16X3: FUSED (kmeans_fused_k).  The n x k scores never reach memory.  A workgroup owns 128 rows (4 waves x 32) and walks d in chunks of 64; every
//     lane loads ITS row's 8 floats of each 16-wide slab straight from HBM (row c = lane & 31, d = 16 s + 8 (lane >> 5) + 0..7: the B operand of
//     v_mfma_f32_32x32x16_bf16, the layout of knn_fused_k's queries), splits them into the three bf16 planes in registers (csrc/split_bf16.h).  The centroids are split ONCE per
//     call (kmeans_prep_k) into "fragment order": the 16 bytes lane l needs for (plane, slab, tile of 32 centroids) sit at
//     ((plane * slabs + slab) * tiles + tile) * 64 + l, so a wave's A operand is one contiguous 1 KB load.  The planes take 6 d k bytes: 12 MB at k = 1024,
//     d = 2048, which every row block finds in L2 / L1; up to the limits (k 4096, d 8192: 192 MB) the indexing is the same and only the reuse is lost - every
//     row block then streams its planes from HBM, correct but slower.  Each (slab, tile) is six products, smallest terms first, into the tile's 32 x 32
//     accumulator; KT <= 8 tiles (256 centroids) are held at once, so x is read from HBM once for k <= 256 and once per block of 256 centroids beyond.
//     The arg-max is ONE compare-select per accumulator element after the last slab (lane (c, h) holds row c's scores of centroids (r & 3) + 8 (r >> 2) + 4 h of
//     each tile, ascending in r: a strict > keeps the lowest index) and one exchange with the partner lane per ROW BLOCK - the vector pipe does not hide behind
//     the matrix pipe (profiles/r02_probe_mfma_plus_valu.txt), so there is nothing per slab.
//   * SSV_ARITH_F32_MFMA: S = X C^T by chunks of rows on the implicit-GEMM kernel into the workspace, then one wavefront per row (kmeans_rowarg_k) - the way
//     ssv_knn_label_agreement_arith falls back.  Same contract.
//   Bit-identical centroid rows give bit-identical scores on both routes (every column runs the same instruction sequence on the same bits), so duplicates never win
//   against their first copy.  counts: integer atomics (order-free).  objective: per-row-block partial sums (fixed tree), folded in double in fixed order.
// Update.  sums = onehot(labels)^T X on the weight-gradient GEMM (products by 1.0 and 0.0 are exact in both arithmetics: only the GEMM's fixed accumulation order
//   rounds; no floating-point atomics), centroid = sums / count, a cluster without members KEEPS its centroid.  A label outside [0, k) contributes to no cluster.
//   The same call re-makes 1/2 |c|^2 and the planes for the next assignment.
#include "common.h"
#include "split_bf16.h"
#include <limits.h>

namespace {

constexpr int MAX_K = SSV_KMEANS_MAX_K, MAX_D = SSV_KMEANS_MAX_D;
constexpr int HIST = 1024;                                       // clusters counted in LDS per workgroup; beyond, rows go to the global counters directly

struct Geo { int T, S4, kpad; size_t hc_bytes, plane_bytes; };  // T tiles of 32 centroids, S4 slabs of 16 columns (a multiple of 4: chunks of 64)
inline Geo geo(int d, int k) {
  Geo g;
  g.T = cdiv(k, 32); g.S4 = cdiv(d, 64) * 4; g.kpad = g.T * 32;
  g.hc_bytes = up256((size_t)g.kpad * 4);
  g.plane_bytes = (size_t)g.S4 * g.T * 1024;
  return g;
}

// blocks [0, S4 * T / 4): the planes in fragment order, one (slab, tile) per wave; blocks behind: hc[j] = 1/2 |c_j|^2 (+inf for the pad of the last tile, whose score
// is then -inf and never chosen), one wave per centroid, lane-strided sum and a fixed xor tree
__global__ void __launch_bounds__(256) kmeans_prep_k(int d, int k, int T, int S4, const float* __restrict__ c, u32x4* __restrict__ planes, float* __restrict__ hc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nfrag = S4 * T;
  const int u = blockIdx.x * 4 + wave;
  if (u < nfrag) {
    const int s = u / T, t = u % T, j = 32 * t + (lane & 31), col = 16 * s + 8 * (lane >> 5);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (j < k) {
      const float* p = c + (int64_t)j * d + col;
      if (col < d) a = *(const f32x4*)p;
      if (col + 4 < d) b = *(const f32x4*)(p + 4);
    }
    bf16x8 pl[3];
    splitbf::split8(a, b, pl);
#pragma unroll
    for (int q = 0; q < 3; ++q) planes[((int64_t)q * nfrag + u) * 64 + lane] = __builtin_bit_cast(u32x4, pl[q]);
    return;
  }
  const int j = u - nfrag;
  if (j >= T * 32) return;
  float ss = 0.f;
  if (j < k)
    for (int e = lane; e < d; e += 64) { const float v = c[(int64_t)j * d + e]; ss = __builtin_fmaf(v, v, ss); }
  ss = wave_sum(ss);
  if (lane == 0) hc[j] = j < k ? 0.5f * ss : INFINITY;
}

__global__ void zero_i32_k(int n, int32_t* p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

// the tail both assignment kernels share: 128 (fused) or 4 (row kernel) rows of a workgroup -> counts and the block's partial objective
template <int ROWS>
__device__ __forceinline__ void block_tail(bool owner, int slot, int label, float dist, int k, int32_t* __restrict__ counts, float* __restrict__ partial, float* sd, int* hist) {
  if (slot >= 0) sd[slot] = owner ? dist : 0.f;
  if (owner) {
    if (k <= HIST) atomicAdd(&hist[label], 1);
    else atomicAdd(&counts[label], 1);
  }
  __syncthreads();
  if (k <= HIST)
    for (int j = threadIdx.x; j < k; j += 256) { const int h = hist[j]; if (h) atomicAdd(&counts[j], h); }
  if (threadIdx.x < 64) {
    float v = 0.f;
    if constexpr (ROWS == 128) v = sd[threadIdx.x] + sd[threadIdx.x + 64];
    else v = (int)threadIdx.x < ROWS ? sd[threadIdx.x] : 0.f;
    v = wave_sum(v);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
  }
}

template <int KT>
__global__ void __launch_bounds__(256, KT >= 4 ? 1 : 2)
kmeans_fused_k(const float* __restrict__ x, const float* __restrict__ cent, int n, int d, int k, int T, int S4, const u32x4* __restrict__ planes, const float* __restrict__ hc,
               int32_t* __restrict__ labels, float* __restrict__ dist, int32_t* __restrict__ counts, float* __restrict__ partial) {
  __shared__ float sd[128];
  __shared__ int hist[HIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  if (k <= HIST)
    for (int j = threadIdx.x; j < k; j += 256) hist[j] = 0;
  const int row = (blockIdx.x * 4 + wave) * 32 + c;
  const float* xp = x + (int64_t)min(row, n - 1) * d + 8 * half;      // rows behind the end repeat the last one and are not written
  const int nch = S4 >> 2;
  const int64_t nfrag = (int64_t)S4 * T;
  auto load_x = [&](int ch, f32x4 (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int col = 64 * ch + 16 * (i >> 1) + 8 * half + 4 * (i & 1);            // d % 4 == 0: a float4 is inside the row or behind it
      r[i] = col < d ? *(const f32x4*)(xp + 64 * ch + 16 * (i >> 1) + 4 * (i & 1)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  float best = -INFINITY;
  int bi = 0;
  for (int tb = 0; tb < T; tb += KT) {                                  // one pass over x per block of KT tiles
    f32x16 acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    int tt[KT];                                                         // tiles behind the last repeat it (their scores are not looked at)
#pragma unroll
    for (int t = 0; t < KT; ++t) tt[t] = min(tb + t, T - 1);
    auto frag = [&](int s, int t, int q) { return __builtin_bit_cast(bf16x8, planes[(q * nfrag + (int64_t)s * T + tt[t]) * 64 + lane]); };
    constexpr int NB = 4, STEPS = 4 * KT;                               // a ring of centroid fragments, three (slab, tile) steps ahead of the products
    bf16x8 kf[NB][3];
#pragma unroll
    for (int st = 0; st < NB - 1; ++st)
#pragma unroll
      for (int q = 0; q < 3; ++q) kf[st][q] = frag(st / KT, st % KT, q);
    f32x4 xr[8];
    load_x(0, xr);
    for (int ch = 0; ch < nch; ++ch) {
      f32x4 xn[8];
      load_x(min(ch + 1, nch - 1), xn);                                 // the last chunk is loaded twice rather than branching around the prefetch
      const int chn = min(ch + 1, nch - 1);
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
          splitbf::mma6_32(acc[t], kf[st % NB], xb);
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[i] = xn[i];
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      if (tb + t < T) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int j0 = 32 * (tb + t) + 8 * g + 4 * half;
          const f32x4 h4 = *(const f32x4*)(hc + j0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float sc = acc[t][4 * g + e] - h4[e];
            const bool up = sc > best;                                  // strict: within a lane the indices ascend, the first maximum stays (NaN never enters)
            best = up ? sc : best;
            bi = up ? j0 + e : bi;
          }
        }
      }
    }
  }
  SSV_ARGMAX_FIRST_STEP(best, bi, 32);                                     // the row's other half
  // the distance to the winner (both halves hold the same bi < k): this half's columns, chunk by chunk - no chain longer than 32 + d / 64 additions
  const float* xq = x + (int64_t)min(row, n - 1) * d;
  const float* cq = cent + (int64_t)bi * d;
  float dsum = 0.f;
#pragma unroll 2
  for (int ch = 0; ch < nch; ++ch) {
    f32x4 xv[8], cv[8];
    bool in[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                        // all sixteen loads before the first use; a float4 behind the row re-reads the row's start instead
      const int col = 64 * ch + 16 * (i >> 1) + 8 * half + 4 * (i & 1);
      in[i] = col < d;                                                   // d % 4 == 0: a float4 is inside the row or behind it
      const int o = in[i] ? col : 0;
      xv[i] = *(const f32x4*)(xq + o);
      cv[i] = *(const f32x4*)(cq + o);
    }
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float df = in[i] ? xv[i][e] - cv[i][e] : 0.f; part = __builtin_fmaf(df, df, part); }
    dsum += part;
  }
  const float dd = dsum + __shfl_xor(dsum, 32, 64);                       // a + b in one lane, b + a in the other: the same float
  const bool owner = half == 0 && row < n;
  if (owner) { labels[row] = bi; dist[row] = dd; }
  __syncthreads();                                                      // hist is zero everywhere
  block_tail<128>(owner, half == 0 ? wave * 32 + c : -1, bi, dd, k, counts, partial, sd, hist);
}

// the unfused route: one wavefront per row of S [rows][k] (chunk of rows from row0), 4 rows per workgroup
__global__ void __launch_bounds__(256) kmeans_rowarg_k(const float* __restrict__ S, int rows, int row0, int d, int k, const float* __restrict__ x, const float* __restrict__ cent, const float* __restrict__ hc,
                                                       int32_t* __restrict__ labels, float* __restrict__ dist, int32_t* __restrict__ counts, float* __restrict__ partial) {
  __shared__ float sd[4];
  __shared__ int hist[HIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (k <= HIST)
    for (int j = threadIdx.x; j < k; j += 256) hist[j] = 0;
  __syncthreads();
  const int r = blockIdx.x * 4 + wave;
  const bool live = r < rows;
  const int rr = live ? r : rows - 1;
  const float* s = S + (int64_t)rr * k;
  float best = -INFINITY;
  int bi = 0;
  for (int j = lane; j < k; j += 64) {
    const float sc = s[j] - hc[j];
    if (sc > best) { best = sc; bi = j; }
  }
  SSV_WAVE_ARGMAX_FIRST(best, bi);
  const float* xp = x + (int64_t)(row0 + rr) * d;
  const float* cp = cent + (int64_t)bi * d;                              // every lane holds the same bi < k
  float ss = 0.f;
  for (int e = lane * 4; e < d; e += 256) {
    const f32x4 v = *(const f32x4*)(xp + e), w = *(const f32x4*)(cp + e);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float df = v[q] - w[q]; ss = __builtin_fmaf(df, df, ss); }
  }
  const float dd = wave_sum(ss);
  const bool owner = live && lane == 0;
  if (owner) { labels[row0 + r] = bi; dist[row0 + r] = dd; }
  block_tail<4>(owner, lane == 0 ? wave : -1, bi, dd, k, counts, partial + row0 / 4, sd, hist);
}

__global__ void __launch_bounds__(256) kmeans_objective_k(int np, const float* __restrict__ partial, float* __restrict__ objective) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) a += (double)partial[i];
  sm[threadIdx.x] = a;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) *objective = (float)sm[0];
}

// onehot [rows][kp] of labels[row0 ..]: one float4 per thread; a label outside [0, k) leaves its row zero
__global__ void __launch_bounds__(256) kmeans_onehot_k(int64_t total4, int kp4, const int32_t* __restrict__ labels, f32x4* __restrict__ oh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t r = i / kp4;
  const int j0 = (int)(i - r * kp4) * 4, l = labels[r];
  oh[i] = f32x4{l == j0 ? 1.f : 0.f, l == j0 + 1 ? 1.f : 0.f, l == j0 + 2 ? 1.f : 0.f, l == j0 + 3 ? 1.f : 0.f};
}

__global__ void __launch_bounds__(256) kmeans_mean_k(int64_t total, int d, const float* __restrict__ sums, const int32_t* __restrict__ counts, float* __restrict__ c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int m = counts[i / d];
  if (m > 0) c[i] = sums[i] / (float)m;                                // an empty cluster keeps its centroid
}

__global__ void __launch_bounds__(256) cluster_votes_k(int64_t n, const int32_t* __restrict__ pred, const int32_t* __restrict__ targets, int pk, int tk,
                                                       unsigned long long* __restrict__ votes, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = pred[i], t = targets[i];
  if ((unsigned)p < (unsigned)pk && (unsigned)t < (unsigned)tk) atomicAdd(&votes[(int64_t)p * tk + t], 1ull);
  else *flag = 1;
}
__global__ void votes_zero_k(int64_t cells, unsigned long long* __restrict__ votes, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < cells) votes[i] = 0ull;
  if (i == 0) *flag = 0;
}

int64_t assign_chunk_rows(int64_t n) { return n < 4096 ? n : 4096; }                 // of S = X C^T on the unfused route (a multiple of 4 unless it is all of n)
int64_t update_chunk_rows(int64_t n, int d, int kp) {                                // rows of one one-hot slab: <= 2^24 one-hot and <= 2^28 x elements per GEMM launch
  int64_t r = (1ll << 24) / kp;
  const int64_t rx = (1ll << 28) / d;
  if (rx < r) r = rx;
  if (r > n) r = n;
  return r < 1 ? 1 : r;
}
bool shape_ok(int64_t n, int32_t d, int32_t k) { return n >= 1 && n <= (1ll << 30) && d >= 1 && d <= MAX_D && k >= 1 && k <= MAX_K && k <= n; }
size_t assign_ws(int64_t n, int d, int k, int arithmetic) {
  size_t b = up256((size_t)cdiv64(n, 4) * 4);                      // the partial objectives of either route
  if (arithmetic != SSV_ARITH_BF16X3) b += (size_t)assign_chunk_rows(n) * k * 4 + 256;
  return b;
}
size_t update_ws(int64_t n, int d, int k, int arithmetic, size_t* sums_bytes, size_t* oh_bytes) {
  const int kp = (k + 3) & ~3;
  const int64_t cr = update_chunk_rows(n, d, kp);
  const size_t sb = up256((size_t)kp * d * 4), ob = up256((size_t)cr * kp * 4);
  ssv_conv_desc a = gemm_conv_desc((int)cr, d, kp, arithmetic), b = gemm_conv_desc((int)(n % cr ? n % cr : cr), d, kp, arithmetic);
  const size_t wa = ssv_conv2d_wgrad_workspace_bytes(&a), wb = ssv_conv2d_wgrad_workspace_bytes(&b);
  if (sums_bytes) *sums_bytes = sb;
  if (oh_bytes) *oh_bytes = ob;
  return sb + ob + (wa > wb ? wa : wb) + 256;
}
int launch_prep(int d, int k, const float* c, void* prep, hipStream_t s) {
  const Geo g = geo(d, k);
  const int units = g.S4 * g.T + g.kpad;
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(kmeans_prep_k, dim3((unsigned)cdiv(units, 4)), dim3(256), 0, s, d, k, g.T, g.S4, c, (u32x4*)((char*)prep + g.hc_bytes), (float*)prep);
  SSV_CHECK_LAUNCH("kmeans_prep_k");
  return SSV_OK;
}

}  // namespace

extern "C" size_t ssv_kmeans_prep_bytes(int32_t d, int32_t k) {
  if (d < 1 || d > MAX_D || k < 1 || k > MAX_K) return 0;
  const Geo g = geo((d + 3) & ~3, k);
  return g.hc_bytes + 3 * g.plane_bytes;
}

extern "C" size_t ssv_kmeans_workspace_bytes(int64_t n, int32_t d, int32_t k, int32_t arithmetic) {
  if (!shape_ok(n, d, k)) return 0;
  d = (d + 3) & ~3;
  const size_t a = assign_ws(n, d, k, arithmetic), u = update_ws(n, d, k, arithmetic, nullptr, nullptr);
  return a > u ? a : u;
}

extern "C" int ssv_kmeans_assign(int64_t n, int32_t d, int32_t k, const float* x, const float* centroids, void* prep, int32_t prep_ready,
                                 int32_t* labels, float* dist, int32_t* counts, float* objective, int32_t arithmetic,
                                 void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(n, d, k), "ssv_kmeans_assign: need 1 <= k <= min(n, %d), 1 <= d <= %d, n <= 2^30 (got n=%lld d=%d k=%d)", MAX_K, MAX_D, (long long)n, d, k);
  SSV_REQUIRE(d % 4 == 0, "ssv_kmeans_assign: d %% 4 == 0 (got %d; pad the columns with zeros, which is exact)", d);
  SSV_REQUIRE(x && centroids && prep && labels && dist && counts && objective && ws, "ssv_kmeans_assign: null pointer");
  SSV_REQUIRE(arithmetic == SSV_ARITH_F32_MFMA || arithmetic == SSV_ARITH_BF16X3, "ssv_kmeans_assign: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE((((uintptr_t)x | (uintptr_t)centroids | (uintptr_t)prep | (uintptr_t)ws) & 15) == 0, "ssv_kmeans_assign: pointers must be 16-byte aligned");
  const size_t need = assign_ws(n, d, k, arithmetic);
  if (ws_bytes < need) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_kmeans_assign: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const Geo g = geo(d, k);
  if (!prep_ready)
    if (int rc = launch_prep(d, k, centroids, prep, s)) return rc;
  const float* hc = (const float*)prep;
  float* partial = (float*)ws;
  int np;
  {
    ProfScope ps(SSV_PROF_MISC, s);
    hipLaunchKernelGGL(zero_i32_k, dim3((unsigned)cdiv(k, 256)), dim3(256), 0, s, k, counts);
  }
  if (arithmetic == SSV_ARITH_BF16X3) {
    ProfScope ps(SSV_PROF_MISC, s);
    const u32x4* planes = (const u32x4*)((const char*)prep + g.hc_bytes);
    np = (int)cdiv64(n, 128);
    const dim3 grid((unsigned)np);
#define SSV_KM(KT) hipLaunchKernelGGL(kmeans_fused_k<KT>, grid, dim3(256), 0, s, x, centroids, (int)n, d, k, g.T, g.S4, planes, hc, labels, dist, counts, partial)
    if (g.T == 1) SSV_KM(1); else if (g.T == 2) SSV_KM(2); else if (g.T <= 4) SSV_KM(4); else SSV_KM(8);
#undef SSV_KM
    SSV_CHECK_LAUNCH("kmeans_fused_k");
  } else {
    float* S = (float*)((char*)ws + up256((size_t)cdiv64(n, 4) * 4));
    const int64_t cr = assign_chunk_rows(n);
    np = (int)cdiv64(n, 4);
    for (int64_t r0 = 0; r0 < n; r0 += cr) {
      const int rows = (int)(n - r0 < cr ? n - r0 : cr);
      ssv_conv_desc cd = gemm_conv_desc(rows, d, k, SSV_ARITH_F32_MFMA);
      if (int rc = ssv_conv2d_fwd(&cd, x + r0 * d, centroids, nullptr, nullptr, S, stream)) return rc;         // S[rows, k] = X[r0 : r0 + rows] C^T
      ProfScope ps(SSV_PROF_MISC, s);
      hipLaunchKernelGGL(kmeans_rowarg_k, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, (const float*)S, rows, (int)r0, d, k, x, centroids, hc, labels, dist, counts, partial);
      SSV_CHECK_LAUNCH("kmeans_rowarg_k");
    }
  }
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(kmeans_objective_k, dim3(1), dim3(256), 0, s, np, (const float*)partial, objective);
  SSV_CHECK_LAUNCH("kmeans_objective_k");
  return SSV_OK;
}

extern "C" int ssv_kmeans_update(int64_t n, int32_t d, int32_t k, const float* x, const int32_t* labels, const int32_t* counts, float* centroids, void* prep,
                                 int32_t arithmetic, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(n, d, k), "ssv_kmeans_update: need 1 <= k <= min(n, %d), 1 <= d <= %d, n <= 2^30 (got n=%lld d=%d k=%d)", MAX_K, MAX_D, (long long)n, d, k);
  SSV_REQUIRE(d % 4 == 0, "ssv_kmeans_update: d %% 4 == 0 (got %d; pad the columns with zeros, which is exact)", d);
  SSV_REQUIRE(x && labels && counts && centroids && ws, "ssv_kmeans_update: null pointer");      // prep may be NULL: nothing is left for a next assignment
  SSV_REQUIRE(arithmetic == SSV_ARITH_F32_MFMA || arithmetic == SSV_ARITH_BF16X3, "ssv_kmeans_update: unknown arithmetic %d", arithmetic);
  SSV_REQUIRE((((uintptr_t)x | (uintptr_t)centroids | (uintptr_t)prep | (uintptr_t)ws) & 15) == 0, "ssv_kmeans_update: pointers must be 16-byte aligned");
  size_t sb = 0, ob = 0;
  const size_t need = update_ws(n, d, k, arithmetic, &sb, &ob);
  if (ws_bytes < need) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_kmeans_update: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const int kp = (k + 3) & ~3;
  float* sums = (float*)ws;
  float* oh = (float*)((char*)ws + sb);
  void* gws = (char*)ws + sb + ob;
  const int64_t cr = update_chunk_rows(n, d, kp);
  for (int64_t r0 = 0; r0 < n; r0 += cr) {
    const int rows = (int)(n - r0 < cr ? n - r0 : cr);
    {
      ProfScope ps(SSV_PROF_MISC, s);
      const int64_t total4 = (int64_t)rows * (kp / 4);
      hipLaunchKernelGGL(kmeans_onehot_k, dim3((unsigned)cdiv64(total4, 256)), dim3(256), 0, s, total4, kp / 4, labels + r0, (f32x4*)oh);
      SSV_CHECK_LAUNCH("kmeans_onehot_k");
    }
    ssv_conv_desc cd = gemm_conv_desc(rows, d, kp, arithmetic);
    if (int rc = ssv_conv2d_wgrad(&cd, x + r0 * d, oh, sums, r0 > 0, gws, ws_bytes - sb - ob, stream)) return rc;   // sums[kp, d] (+)= onehot^T X, chunks in row order
  }
  {
    ProfScope ps(SSV_PROF_MISC, s);
    const int64_t total = (int64_t)k * d;
    hipLaunchKernelGGL(kmeans_mean_k, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, total, d, (const float*)sums, counts, centroids);
    SSV_CHECK_LAUNCH("kmeans_mean_k");
  }
  if (prep) return launch_prep(d, k, centroids, prep, s);
  return SSV_OK;
}

extern "C" int ssv_cluster_votes(int64_t n, const int32_t* pred, const int32_t* targets, int32_t pred_k, int32_t targets_k, int64_t* votes, int32_t* flag,
                                 void* stream) {
  SSV_REQUIRE(n >= 1 && n < (1ll << 31) && pred_k >= 1 && targets_k >= 1 && (int64_t)pred_k * targets_k <= (1ll << 24),
              "ssv_cluster_votes: need 1 <= n < 2^31 and 1 <= pred_k * targets_k <= 2^24 (got n=%lld pred_k=%d targets_k=%d)", (long long)n, pred_k, targets_k);
  SSV_REQUIRE(pred && targets && votes && flag, "ssv_cluster_votes: null pointer");
  SSV_REQUIRE(((uintptr_t)votes & 7) == 0 && (const void*)votes != (const void*)pred && (const void*)votes != (const void*)targets && (const void*)flag != (const void*)votes,
              "ssv_cluster_votes: votes must be 8-byte aligned and alias neither the labels nor the flag");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  const int64_t cells = (int64_t)pred_k * targets_k;
  hipLaunchKernelGGL(votes_zero_k, dim3((unsigned)cdiv64(cells, 256)), dim3(256), 0, s, cells, (unsigned long long*)votes, flag);
  hipLaunchKernelGGL(cluster_votes_k, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, n, pred, targets, pred_k, targets_k, (unsigned long long*)votes, flag);
  SSV_CHECK_LAUNCH("ssv_cluster_votes");
  return SSV_OK;
}
