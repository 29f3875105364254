// The weighted kNN classifier (InstDisc, MoCo, DINO's eval_knn): an exact inner-product top-k search of a query matrix against a bank, and the temperature-weighted class
// vote over its result.  The reference has neither (its compute_neighbor_accuracy searches a set against itself, csrc/evalknn.hip).  Contract: include/ssv_hip.h.
//
// Search.  S = Q B^T is formed chunk by chunk in the workspace by the implicit-GEMM kernel (a part of the bank as a 1x1 filter bank, the way ssv_knn_label_agreement_arith
//   and the f32 route of ssv_kmeans_assign do it), in either arithmetic; then ONE WORKGROUP per row of the chunk selects (knn_select_k):
//   * a score becomes an order-preserving 32-bit key (sign flip; -0 as +0; every NaN the key 0, below -inf);
//   * radix select, most significant digit first: four passes of 8-bit digits, each a histogram of integer counts in LDS over the keys that still match the prefix
//     (16 copies of the 256 bins, one per lane & 15: scores of unit vectors share their top digit, and 64 lanes on one counter would serialise).  After the passes the
//     k-th key is known, and with it how many keys are strictly greater and how many equal ones are still missing;
//   * one pass gathers the strictly greater entries (an LDS cursor: their order is settled by the sort) and counts the equal ones per wave; the equal ones that are
//     taken are the LOWEST indices: every wave owns a contiguous quarter of the row, so ballots give an equal entry its rank in index order, and a wave stops as soon as
//     nothing is missing - without ties that is one wave reading up to the k-th entry;
//   * the <= 1024 (key, ~index) pairs are sorted descending by a bitonic network in LDS: key descending, index ascending.  sim is read back from S: the product's own bits.
//   The cost per row is six passes at most, whatever k is.  No floating-point atomics, no order-dependent result: equal inputs give equal bits.
//   A bank wider than one part: every part yields its sorted top-min(k, columns) and knn_merge_k merges it into the running result in place (both lists in LDS, the rank
//   of an entry = its position + the entries of the other list that precede it, by binary search).
// Vote (knn_vote_k).  One workgroup per query: the k weights expf((sim_r - sim_0) / T) and labels go to LDS once, then one THREAD per class walks them in rank order - a
//   fixed summation order without atomics - and topn rounds of a workgroup arg-max (score descending, lower class on a tie) give the predictions.
#include "common.h"
#include <limits.h>

namespace {

constexpr int MAX_K = SSV_KNN_MAX_K, MAX_D = SSV_KNN_MAX_D, MAX_C = SSV_KNN_MAX_CLASSES, MAX_TOPN = SSV_KNN_MAX_TOPN;
constexpr int COPIES = 16;                                              // histogram copies (lane & 15)
constexpr int DEFAULT_CHUNK_ROWS = 1024, MAX_PART_COLS = 65536;
constexpr int64_t PART_ELEMS = 1ll << 26;                               // part_cols * d of the default partition: 384 MiB of bf16 planes
constexpr int64_t GEMM_ELEMS = (1ll << 29) - (1ll << 22);               // check_desc of conv_mfma.hip: activations and outputs of one launch

typedef unsigned long long u64;

// ascending in the search's order: NaN (0) < -inf < ... < -0 == +0 < ... < +inf
__device__ __forceinline__ uint32_t key_of(float v) {
  uint32_t u = __float_as_uint(v);
  u = u == 0x80000000u ? 0u : u;
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return v != v ? 0u : k;
}
// descending in the result's order: key descending, index ascending (indices are distinct, so are the pairs; 0 is no pair)
__device__ __forceinline__ u64 pair_of(uint32_t key, int j) { return ((u64)key << 32) | (uint32_t)~(uint32_t)j; }
__device__ __forceinline__ int index_of(u64 p) { return (int)~(uint32_t)p; }

template <bool VEC>
__global__ void __launch_bounds__(256) knn_select_k(const float* __restrict__ S, int cols, int kk, int col0, float* __restrict__ out_sim, int32_t* __restrict__ out_idx, int ld) {
  __shared__ int hist[256 * COPIES];
  __shared__ u64 buf[MAX_K];
  __shared__ int cnt[256];
  __shared__ int sel[2], weq[4], ngt;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* s = S + (int64_t)blockIdx.x * cols;
  out_sim += (int64_t)blockIdx.x * ld;
  out_idx += (int64_t)blockIdx.x * ld;
  const int seg = (((cols + 3) >> 2) + 255) & ~255;                     // a wave's quarter of the row: whole trips of 64 lanes x 4 columns
  const int64_t beg64 = (int64_t)wave * seg;
  const int beg = beg64 < cols ? (int)beg64 : cols, end = (int64_t)beg + seg < cols ? beg + seg : cols;
  // keys of columns j .. j + 3 of this wave's quarter; returns how many of them exist (VEC: cols % 4 == 0, so 0 or 4 and the row is 16-byte aligned)
  auto load4 = [&](int j, uint32_t (&key)[4]) {
    int nv = end - j;
    nv = nv < 0 ? 0 : nv > 4 ? 4 : nv;
    if constexpr (VEC) {
      if (nv) {
        const f32x4 x = *(const f32x4*)(s + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) key[e] = key_of(x[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nv) key[e] = key_of(s[j + e]);
    }
    return nv;
  };
  if (t == 0) ngt = 0;
  uint32_t prefix = 0, mask = 0;
  int need = kk;                                                         // the rank of the wanted key among the keys that match the prefix (1 = the largest)
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < 256 * COPIES; i += 256) hist[i] = 0;
    __syncthreads();
    for (int j0 = beg; j0 < end; j0 += 256) {
      uint32_t key[4];
      const int nv = load4(j0 + 4 * lane, key);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nv && (key[e] & mask) == prefix) atomicAdd(&hist[((key[e] >> shift) & 255) * COPIES + (lane & (COPIES - 1))], 1);
    }
    __syncthreads();
    {
      int c = 0;
#pragma unroll
      for (int q = 0; q < COPIES; ++q) c += hist[t * COPIES + ((q + t) & (COPIES - 1))];
      cnt[t] = c;
    }
    __syncthreads();
    if (t < 64) {                                                       // lane l: bins 255 - 4 l downwards; a scan from the top finds the bin that holds rank `need`
      const int b0 = 255 - 4 * t;
      int c[4], tot = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { c[e] = cnt[b0 - e]; tot += c[e]; }
      int incl = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      int run = incl - tot;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (run < need && need <= run + c[e]) { sel[0] = b0 - e; sel[1] = run; }
        run += c[e];
      }
    }
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    mask |= 255u << shift;
    need -= sel[1];
  }
  const uint32_t kth = prefix;
  const int greater = kk - need;                                        // keys strictly above the k-th; `need` >= 1 entries equal to it are taken
  int eq_w = 0;
  for (int j0 = beg; j0 < end; j0 += 256) {
    uint32_t key[4];
    const int j = j0 + 4 * lane, nv = load4(j, key);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nv && key[e] > kth) buf[atomicAdd(&ngt, 1)] = pair_of(key[e], j + e);
      eq_w += __popcll(__ballot(e < nv && key[e] == kth));
    }
  }
  if (lane == 0) weq[wave] = eq_w;
  __syncthreads();
  int run = 0;
  for (int w = 0; w < wave; ++w) run += weq[w];                         // equal entries in the quarters before this wave's
  if (eq_w > 0 && run < need) {                                         // wave-uniform
    const u64 below_mask = (1ull << lane) - 1ull;
    const int last = run + eq_w;
    for (int j0 = beg; j0 < end && run < need && run < last; j0 += 256) {
      uint32_t key[4];
      const int j = j0 + 4 * lane, nv = load4(j, key);
      int below = 0, all = 0;
      bool eq[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        eq[e] = e < nv && key[e] == kth;
        const u64 b = __ballot(eq[e]);
        below += __popcll(b & below_mask);
        all += __popcll(b);
      }
      int r = run + below;                                              // index order: the lower lanes' four columns first, then this lane's own
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (eq[e]) {
          if (r < need) buf[greater + r] = pair_of(kth, j + e);
          ++r;
        }
      }
      run += all;
    }
  }
  int P = 1;
  while (P < kk) P <<= 1;
  __syncthreads();
  for (int i = kk + t; i < P; i += 256) buf[i] = 0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (P >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const u64 a = buf[lo], b = buf[hi];
        if ((a < b) == desc) { buf[lo] = b; buf[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (int i = t; i < kk; i += 256) {
    const int j = index_of(buf[i]);
    out_idx[i] = col0 + j;
    out_sim[i] = s[j];
  }
}

// sim / idx [row][0 .. la) (the running result) and tsim / tidx [row][0 .. lb) (a part's), both sorted -> the best kout of their union, in place
__global__ void __launch_bounds__(256) knn_merge_k(float* __restrict__ sim, int32_t* __restrict__ idx, int ld, int la, const float* __restrict__ tsim,
                                                   const int32_t* __restrict__ tidx, int lb, int kout) {
  __shared__ u64 pa[MAX_K], pb[MAX_K];
  __shared__ float va[MAX_K], vb[MAX_K];
  const int t = threadIdx.x;
  sim += (int64_t)blockIdx.x * ld; idx += (int64_t)blockIdx.x * ld;
  tsim += (int64_t)blockIdx.x * ld; tidx += (int64_t)blockIdx.x * ld;
  for (int i = t; i < la; i += 256) { const float v = sim[i]; va[i] = v; pa[i] = pair_of(key_of(v), idx[i]); }
  for (int i = t; i < lb; i += 256) { const float v = tsim[i]; vb[i] = v; pb[i] = pair_of(key_of(v), tidx[i]); }
  __syncthreads();                                                       // every read of the running result is done before the first write
  auto ahead = [](const u64* list, int len, u64 p) {                     // entries of a descending list that precede p
    int lo = 0, hi = len;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (list[mid] > p) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  for (int i = t; i < la; i += 256) {
    const int r = i + ahead(pb, lb, pa[i]);
    if (r < kout) { sim[r] = va[i]; idx[r] = index_of(pa[i]); }
  }
  for (int i = t; i < lb; i += 256) {
    const int r = i + ahead(pa, la, pb[i]);
    if (r < kout) { sim[r] = vb[i]; idx[r] = index_of(pb[i]); }
  }
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    const u64 other = ((u64)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

__global__ void knn_flag_zero_k(int32_t* flag) { *flag = 0; }

__global__ void __launch_bounds__(256) knn_vote_k(int k, int64_t n, int C, int topn, const float* __restrict__ sim, const int32_t* __restrict__ idx,
                                                  const int32_t* __restrict__ labels, float inv_temp, int32_t* __restrict__ pred, float* __restrict__ scores,
                                                  int32_t* __restrict__ flag) {
  __shared__ float w[MAX_K];
  __shared__ int lab[MAX_K];
  __shared__ u64 rank[MAX_C];                                            // (key of the score, ~class): the arg-max order; 0 once a class is taken
  __shared__ u64 wm[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  sim += (int64_t)blockIdx.x * k; idx += (int64_t)blockIdx.x * k;
  const float s0 = sim[0];
  for (int r = t; r < k; r += 256) {
    const float v = sim[r];
    const int j = idx[r];
    int l = -1;
    if (j >= 0 && (int64_t)j < n) {
      l = labels[j];
      if ((unsigned)l >= (unsigned)C) { l = -1; *flag = 1; }
    } else {
      *flag = 1;
    }
    w[r] = expf((v - s0) * inv_temp);
    lab[r] = v != v ? -1 : l;                                           // a NaN similarity votes for nobody
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    float acc = 0.f;
    for (int r = 0; r < k; ++r) acc = lab[r] == c ? acc + w[r] : acc;     // rank order
    if (scores) scores[(int64_t)blockIdx.x * C + c] = acc;
    rank[c] = pair_of(key_of(acc), c);
  }
  __syncthreads();
  for (int round = 0; round < topn; ++round) {
    u64 best = 0ull;
    for (int c = t; c < C; c += 256) best = rank[c] > best ? rank[c] : best;
    best = wave_max_u64(best);
    if (lane == 0) wm[wave] = best;
    __syncthreads();
    if (t == 0) {
      u64 b = wm[0];
#pragma unroll
      for (int q = 1; q < 4; ++q) b = wm[q] > b ? wm[q] : b;
      const int c = index_of(b);
      pred[(int64_t)blockIdx.x * topn + round] = c;
      rank[c] = 0ull;
    }
    __syncthreads();
  }
}

// ---- the partition of one search ------------------------------------------------------------------------------------------------------------------------------------
struct Plan { int cr, pc, arith; size_t s_bytes, planes_bytes, tmp_bytes; };

// false (with the reason in `why`, if given) for what ssv_knn_search refuses
bool make_plan(int64_t m, int64_t n, int32_t d, int32_t k, int32_t arithmetic, int32_t chunk_rows, int32_t part_cols, Plan* p, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "need 1 <= m <= 2^30, 1 <= n < 2^31, 1 <= k <= min(n, 1024), d % 4 == 0, 4 <= d <= 8192";
  if (m < 1 || m > (1ll << 30) || n < 1 || n >= (1ll << 31) || d < 4 || d > MAX_D || d % 4 != 0 || k < 1 || k > MAX_K || k > n) return false;
  *why = "unknown arithmetic";
  if (arithmetic != SSV_ARITH_F32_MFMA && arithmetic != SSV_ARITH_BF16X3) return false;
  *why = "chunk_rows and part_cols must not be negative (0: the library's choice)";
  if (chunk_rows < 0 || part_cols < 0) return false;
  int64_t pc = part_cols;
  if (pc == 0) {                                                         // equal parts of at most min(65536, 2^26 / d) columns, whole float4s
    int64_t cap = PART_ELEMS / d;
    if (cap > MAX_PART_COLS) cap = MAX_PART_COLS;
    const int64_t parts = cdiv64(n, cap);
    pc = (cdiv64(n, parts) + 3) & ~(int64_t)3;
  }
  if (pc > n) pc = n;                                                    // one part
  int64_t cr = chunk_rows ? chunk_rows : DEFAULT_CHUNK_ROWS;
  if (cr > m) cr = m;                                                    // one chunk
  *why = "a chunk of S breaks the GEMM's limits: chunk_rows * part_cols and chunk_rows * d below 2^29 - 2^22, part_cols * d below 2^29";
  if (cr * pc >= GEMM_ELEMS || cr * d >= GEMM_ELEMS || pc * d >= (1ll << 29)) return false;
  p->cr = (int)cr; p->pc = (int)pc;
  // bf16 pieces: whole 32-channel k-tiles and 16-byte rows of every part of S (conv_mfma.hip: sp_fwd_ok); otherwise the whole call runs on fp32 MFMA
  p->arith = (arithmetic == SSV_ARITH_BF16X3 && d % 32 == 0 && pc % 4 == 0 && n % 4 == 0 && pc * d * 6 < (1ll << 31)) ? SSV_ARITH_BF16X3 : SSV_ARITH_F32_MFMA;
  p->s_bytes = up256((size_t)cr * pc * 4);
  p->planes_bytes = p->arith == SSV_ARITH_BF16X3 ? up256((size_t)pc * d * 6) : 0;
  p->tmp_bytes = up256((size_t)cr * k * 4);                             // twice: a part's sim and idx
  return true;
}

}  // namespace

extern "C" size_t ssv_knn_search_workspace_bytes(int64_t m, int64_t n, int32_t d, int32_t k, int32_t arithmetic, int32_t chunk_rows, int32_t part_cols) {
  Plan p;
  if (!make_plan(m, n, d, k, arithmetic, chunk_rows, part_cols, &p, nullptr)) return 0;
  return p.s_bytes + p.planes_bytes + 2 * p.tmp_bytes;
}

extern "C" int ssv_knn_search(int64_t m, int64_t n, int32_t d, int32_t k, const float* queries, const float* bank, float* sim, int32_t* idx,
                              int32_t arithmetic, int32_t chunk_rows, int32_t part_cols, void* ws, size_t ws_bytes, void* stream) {
  Plan p;
  const char* why = "";
  SSV_REQUIRE(make_plan(m, n, d, k, arithmetic, chunk_rows, part_cols, &p, &why), "ssv_knn_search: %s (got m=%lld n=%lld d=%d k=%d arithmetic=%d chunk_rows=%d part_cols=%d)",
              why, (long long)m, (long long)n, d, k, arithmetic, chunk_rows, part_cols);
  SSV_REQUIRE(queries && bank && sim && idx && ws, "ssv_knn_search: null pointer");
  SSV_REQUIRE((((uintptr_t)queries | (uintptr_t)bank | (uintptr_t)ws) & 15) == 0 && (((uintptr_t)sim | (uintptr_t)idx) & 3) == 0, "ssv_knn_search: queries, bank and ws must be 16-byte aligned");
  SSV_REQUIRE((const void*)sim != (const void*)idx && (const void*)sim != (const void*)queries && (const void*)sim != (const void*)bank &&
              (const void*)idx != (const void*)queries && (const void*)idx != (const void*)bank, "ssv_knn_search: sim and idx alias neither each other nor an input");
  const size_t need = p.s_bytes + p.planes_bytes + 2 * p.tmp_bytes;
  if (ws_bytes < need) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_knn_search: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  float* S = (float*)ws;
  void* planes = p.planes_bytes ? (char*)ws + p.s_bytes : nullptr;
  float* tsim = (float*)((char*)ws + p.s_bytes + p.planes_bytes);
  int32_t* tidx = (int32_t*)((char*)tsim + p.tmp_bytes);
  int64_t have = 0;                                                     // entries of the running result: min(k, columns searched so far)
  for (int64_t c0 = 0; c0 < n; c0 += p.pc) {
    const int cols = (int)(n - c0 < p.pc ? n - c0 : p.pc);
    const int kk = k < cols ? k : cols;
    const int64_t kout = have + kk < k ? have + kk : k;
    if (planes)
      if (int rc = ssv_split_planes((int64_t)cols * d, bank + c0 * d, planes, stream)) return rc;
    for (int64_t r0 = 0; r0 < m; r0 += p.cr) {
      const int rows = (int)(m - r0 < p.cr ? m - r0 : p.cr);
      ssv_conv_desc cd = gemm_conv_desc(rows, d, cols, p.arith, planes);
      if (int rc = ssv_conv2d_fwd(&cd, queries + r0 * d, bank + c0 * d, nullptr, nullptr, S, stream)) return rc;      // S[rows, cols] = Q[r0 : r0 + rows] B[c0 : c0 + cols]^T
      ProfScope ps(SSV_PROF_MISC, s);
      float* osim = c0 == 0 ? sim + r0 * k : tsim;
      int32_t* oidx = c0 == 0 ? idx + r0 * k : tidx;
      if (cols % 4 == 0) hipLaunchKernelGGL(knn_select_k<true>, dim3((unsigned)rows), dim3(256), 0, s, (const float*)S, cols, kk, (int)c0, osim, oidx, k);
      else hipLaunchKernelGGL(knn_select_k<false>, dim3((unsigned)rows), dim3(256), 0, s, (const float*)S, cols, kk, (int)c0, osim, oidx, k);
      SSV_CHECK_LAUNCH("knn_select_k");
      if (c0 > 0) {
        hipLaunchKernelGGL(knn_merge_k, dim3((unsigned)rows), dim3(256), 0, s, sim + r0 * k, idx + r0 * k, k, (int)have, (const float*)tsim, (const int32_t*)tidx, kk, (int)kout);
        SSV_CHECK_LAUNCH("knn_merge_k");
      }
    }
    have = kout;
  }
  return SSV_OK;
}

extern "C" int ssv_knn_vote(int64_t m, int32_t k, int64_t n, int32_t num_classes, int32_t topn, const float* sim, const int32_t* idx, const int32_t* bank_labels,
                            float inv_temp, int32_t* pred, float* scores, int32_t* flag, void* stream) {
  SSV_REQUIRE(m >= 1 && m <= (1ll << 30) && k >= 1 && k <= MAX_K && n >= 1 && n < (1ll << 31) && num_classes >= 1 && num_classes <= MAX_C,
              "ssv_knn_vote: need 1 <= m <= 2^30, 1 <= k <= %d, 1 <= n < 2^31, 1 <= num_classes <= %d (got m=%lld k=%d n=%lld num_classes=%d)", MAX_K, MAX_C, (long long)m, k,
              (long long)n, num_classes);
  SSV_REQUIRE(topn >= 1 && topn <= MAX_TOPN && topn <= num_classes, "ssv_knn_vote: need 1 <= topn <= min(num_classes, %d) (got topn=%d, num_classes=%d)", MAX_TOPN, topn, num_classes);
  SSV_REQUIRE(inv_temp > 0.f && inv_temp <= 3.0e38f, "ssv_knn_vote: inv_temp must be finite and positive (got %g)", (double)inv_temp);
  SSV_REQUIRE(sim && idx && bank_labels && pred && flag, "ssv_knn_vote: null pointer");
  SSV_REQUIRE((((uintptr_t)sim | (uintptr_t)idx | (uintptr_t)bank_labels | (uintptr_t)pred | (uintptr_t)scores | (uintptr_t)flag) & 3) == 0, "ssv_knn_vote: pointers must be 4-byte aligned");
  const void* in[3] = {sim, idx, bank_labels};
  const void* out[3] = {pred, flag, scores};
  for (int a = 0; a < 3; ++a) {
    if (!out[a]) continue;
    for (int b = 0; b < 3; ++b) SSV_REQUIRE(out[a] != in[b], "ssv_knn_vote: pred, scores and flag alias neither each other nor an input");
    for (int b = a + 1; b < 3; ++b) SSV_REQUIRE(out[a] != out[b], "ssv_knn_vote: pred, scores and flag alias neither each other nor an input");
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(knn_flag_zero_k, dim3(1), dim3(1), 0, s, flag);
  hipLaunchKernelGGL(knn_vote_k, dim3((unsigned)m), dim3(256), 0, s, k, n, num_classes, topn, sim, idx, bank_labels, inv_temp, pred, scores, flag);
  SSV_CHECK_LAUNCH("ssv_knn_vote");
  return SSV_OK;
}
