// The batched whitening of W-MSE (Ermolov et al., ICML 2021): centring, covariance, Cholesky factor and triangular inverse of many small blocks of rows, and the
// backward of all of it.  The contract is in include/ssv_hip.h (ssv_whiten_fwd / ssv_whiten_bwd / ssv_wmse_perm).
//
//   * ONE WORKGROUP of 1024 threads PER BLOCK; the d x d matrices live in LDS with a row stride of d + 1 words (column walks and row walks are both free of bank
//     conflicts), the rows of x are gathered in chunks of 32 (forward) or 16 (backward) rows through LDS.  The LDS footprint is a function of d (lds_layout); the
//     kernels are instantiated for 16 KiB, 64 KiB and the whole 160 KiB of a CU.
//   * Every sum runs in double in a fixed order: the column means by P row classes folded in order, the d x d products of w terms in 4 x 4 register tiles whose
//     k-split (small d) is folded through LDS in ascending order, the dot products of the factorisation over 8 lanes joined by an xor butterfly (every lane
//     obtains the same bits).  No atomics.
//   * forward: mean -> A = (1 - eps) xc^T xc / (w - 1) + eps I -> one loop of d + 1 phases with ONE barrier each: phase j computes column j of L (left-looking:
//     reads columns < j) and row j - 1 of W = L^-1 (forward substitution: reads row j - 1 of L and rows < j - 1 of W), every thread re-deriving the pivot so that no
//     second barrier is needed to publish it -> y = xc W^T.  The centred rows go to the workspace on the first pass and are read from there on the second.
//   * backward: no L is needed.  With M = dW W^T (dW = G^T xc), L^T dL = -M on the lower triangle, so dA = -sym(W^T Phi(M) W); the three d x d products run in
//     place in one LDS buffer (every thread holds its <= 16 outputs in registers across a barrier), and because xc has zero column sums the column mean of g is
//     that of G W: dx = (G - colmean G) W + 2 (1 - eps) / (w - 1) xc dA.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {

constexpr int NT = 1024;                       // threads of a workgroup
constexpr int FCH = 32, BCH = 16;              // rows of one staged chunk: forward, backward (two operands)
constexpr int MAX_D = SSV_WHITEN_MAX_D, MAX_W = SSV_WHITEN_MAX_W;
constexpr uint32_t PERM_VIEW_BASE = 2048;      // Philox view key of iteration t: PERM_VIEW_BASE + t (the augmentation streams use 0 .. 1024 + views)

struct Lay { int ld, kp, P; uint32_t b1, sd, xs, gs, mu, gb, part, dg, total; };

// byte offsets of the LDS sections for width d: B0 | B1 | Sd (double, only with a k-split) | xs | gs (backward) | mu | gb | part | dg
__host__ __device__ inline Lay lds_layout(int d, int ch, bool bwd) {
  Lay l;
  l.ld = d + 1;
  const int T = (d / 4) * (d / 4);
  int kp = 1;
  while (kp < 16 && 2 * kp * T <= NT) kp *= 2;
  l.kp = kp;
  int P = NT / d;
  l.P = P > 16 ? 16 : P;
  const uint32_t mat = ((uint32_t)d * l.ld * 4 + 15) & ~15u, chunk = ((uint32_t)ch * l.ld * 4 + 15) & ~15u;
  uint32_t o = 0;
  o += mat; l.b1 = o;
  o += mat; l.sd = o;
  o += kp > 1 ? (uint32_t)d * d * 8 : 0; l.xs = o;
  o += chunk; l.gs = o;
  o += bwd ? chunk : 0; l.mu = o;
  o += (uint32_t)d * 4; l.gb = o;
  o += (uint32_t)d * 8; l.part = o;
  o += (uint32_t)l.P * d * 8; l.dg = o;
  o += (uint32_t)d * 4; l.total = o;
  return l;
}

__device__ __forceinline__ double group8_sum(double v) {
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// column means of `rows` rows of width d in double: src(i) -> pointer to row i.  part: P * d doubles; out[j] for j < d.  Ends with a barrier.
template <class RowPtr>
__device__ __forceinline__ void column_means(int w, int d, int P, RowPtr src, double* part, double* out) {
  const int p = threadIdx.x / d, j = threadIdx.x % d;
  if (p < P) {
    double a = 0.0;
    for (int i = p; i < w; i += P) a += (double)src(i)[j];
    part[p * d + j] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < d) {
    double s = 0.0;
    for (int q = 0; q < P; ++q) s += part[q * d + threadIdx.x];
    out[threadIdx.x] = s / (double)w;
  }
  __syncthreads();
}

// dst[(i, j)] = f(i, j) for the whole d x d matrix where f reads dst itself: every thread keeps its outputs in registers across a barrier.  Ends with a barrier.
template <class F>
__device__ __forceinline__ void inplace_dxd(float* dst, int d, int ld, F f) {
  float r[MAX_D * MAX_D / NT];
#pragma unroll
  for (int m = 0; m < MAX_D * MAX_D / NT; ++m) {
    const int o = threadIdx.x + NT * m;
    r[m] = o < d * d ? f(o / d, o % d) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MAX_D * MAX_D / NT; ++m) {
    const int o = threadIdx.x + NT * m;
    if (o < d * d) dst[(o / d) * ld + o % d] = r[m];
  }
  __syncthreads();
}

// out[a][b] = sum over the w rows of the block of A_i[a] * B_i[b] in 4 x 4 register tiles (double), the rows staged chunk by chunk: stage(c0, nr) fills as / bs
// (row stride ld) and ends with a barrier.  With a k-split the partial tiles are folded through Sd in ascending order.  emit(a, b, sum) consumes the result.
template <class Stage, class Emit>
__device__ __forceinline__ void gram_dxd(int w, int d, int ld, int kp, int ch, const float* as, const float* bs, double* Sd, Stage stage, Emit emit) {
  const int nt = d / 4, T = nt * nt;
  const int tile = threadIdx.x % T, kpi = threadIdx.x / T;
  const bool active = kpi < kp;
  const int ti = tile / nt, tj = tile % nt;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int c0 = 0; c0 < w; c0 += ch) {
    const int nr = w - c0 < ch ? w - c0 : ch;
    stage(c0, nr);
    if (active)
      for (int r = kpi; r < nr; r += kp) {
        double a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = (double)as[r * ld + 4 * ti + k]; b[k] = (double)bs[r * ld + 4 * tj + k]; }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fma(a[p], b[q], acc[p][q]);
      }
    __syncthreads();
  }
  if (kp == 1) {
    if (active)
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) emit(4 * ti + p, 4 * tj + q, acc[p][q]);
    __syncthreads();
    return;
  }
  for (int k = 0; k < kp; ++k) {                                         // ascending: the order of the additions is part of the result
    if (active && kpi == k)
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double* s = Sd + (4 * ti + p) * d + 4 * tj + q;
          *s = k == 0 ? acc[p][q] : *s + acc[p][q];
        }
    __syncthreads();
  }
  for (int o = threadIdx.x; o < d * d; o += NT) emit(o / d, o % d, Sd[o]);
  __syncthreads();
}

// flag: one int of LDS.  Ends with a barrier.
__device__ __forceinline__ bool rows_in_range(int w, int n_rows, const int32_t* __restrict__ rb, int* flag) {
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  int bad = 0;
  for (int i = threadIdx.x; i < w; i += NT) { const int r = rb[i]; bad |= (r < 0 || r >= n_rows) ? 1 : 0; }
  if (bad) *flag = 1;                                                     // every writer stores the same value
  __syncthreads();
  const bool ok = *flag == 0;
  __syncthreads();
  return ok;
}

template <int LDSB>
__global__ void __launch_bounds__(NT)
whiten_fwd_k(int w, int d, int n_rows, const float* __restrict__ x, const int32_t* __restrict__ rows, float eps, float* __restrict__ y, float* __restrict__ mean,
             float* __restrict__ winv, int32_t* __restrict__ info, float* __restrict__ xcws) {
  __shared__ __align__(16) unsigned char sm[LDSB];
  const Lay L = lds_layout(d, FCH, false);
  float* Lm = (float*)sm;
  float* Wm = (float*)(sm + L.b1);
  double* Sd = (double*)(sm + L.sd);
  float* xs = (float*)(sm + L.xs);
  float* muf = (float*)(sm + L.mu);
  double* mud = (double*)(sm + L.gb);
  double* part = (double*)(sm + L.part);
  float* dg = (float*)(sm + L.dg);
  const int b = blockIdx.x, tid = threadIdx.x, ld = L.ld, d4 = d / 4;
  const int32_t* rb = rows + (int64_t)b * w;
  float* yb = y + (int64_t)b * w * d;
  float* xcb = xcws + (int64_t)b * w * d;
  float* wb = winv + (int64_t)b * d * d;
  float* mb = mean + (int64_t)b * d;
  const float qnan = __builtin_nanf("");
  auto fill_nan = [&](bool with_mean) {
    for (int o = tid; o < w * d; o += NT) yb[o] = qnan;
    for (int o = tid; o < d * d; o += NT) wb[o] = qnan;
    if (with_mean && tid < d) mb[tid] = qnan;
  };
  if (!rows_in_range(w, n_rows, rb, (int*)(sm + L.dg))) {                  // nothing of x is read
    fill_nan(true);
    if (tid == 0) info[b] = -1;
    return;
  }
  column_means(w, d, L.P, [&](int i) { return x + (int64_t)rb[i] * d; }, part, mud);
  if (tid < d) { muf[tid] = (float)mud[tid]; mb[tid] = muf[tid]; }
  __syncthreads();
  // A = (1 - eps) xc^T xc / (w - 1) + eps I  (both triangles, bit-symmetric: the two products of a pair commute)
  const double cs = (1.0 - (double)eps) / (double)(w - 1);
  gram_dxd(w, d, ld, L.kp, FCH, xs, xs, Sd,
           [&](int c0, int nr) {
             for (int q = tid; q < nr * d4; q += NT) {
               const int r = q / d4, c = 4 * (q % d4);
               const f32x4 v = *(const f32x4*)(x + (int64_t)rb[c0 + r] * d + c);
               f32x4 o;
#pragma unroll
               for (int k = 0; k < 4; ++k) { o[k] = v[k] - muf[c + k]; xs[r * ld + c + k] = o[k]; }
               *(f32x4*)(xcb + (int64_t)(c0 + r) * d + c) = o;
             }
             __syncthreads();
           },
           [&](int a, int c, double s) { Lm[a * ld + c] = (float)(cs * s + (a == c ? (double)eps : 0.0)); });
  // phase j: column j of L below the diagonal (the diagonal of L goes to dg; Lm keeps A's), row j - 1 of W
  const int i = tid >> 3, s = tid & 7;
  int fail = 0;
  for (int j = 0; j <= d; ++j) {
    if (j < d) {
      const float* lj = Lm + j * ld;
      const float* li = Lm + (i < d ? i : 0) * ld;
      double ap = 0.0, ar = 0.0;
      for (int k = s; k < j; k += 8) {
        const double pv = (double)lj[k];
        ap = __builtin_fma(pv, pv, ap);
        ar = __builtin_fma((double)li[k], pv, ar);
      }
      ap = group8_sum(ap);
      ar = group8_sum(ar);
      const float piv = (float)((double)lj[j] - ap);                        // the same bits in every thread
      if (!(piv > 0.f && piv < INFINITY)) { fail = j + 1; break; }
      const float ljj = sqrtf(piv);
      if (s == 0 && i < d) {
        if (i == j) dg[j] = ljj;
        else if (i > j) Lm[i * ld + j] = (float)(((double)li[j] - ar) / (double)ljj);
      }
    }
    if (j >= 1) {
      const int r = j - 1, c = i;
      double a = 0.0;
      if (c < r)
        for (int k = c + s; k < r; k += 8) a = __builtin_fma((double)Lm[r * ld + k], (double)Wm[k * ld + c], a);
      a = group8_sum(a);
      if (s == 0 && c < d) Wm[r * ld + c] = c > r ? 0.f : (float)(((c == r ? 1.0 : 0.0) - a) / (double)dg[r]);
    }
    __syncthreads();
  }
  if (fail) {                                                             // uniform: every thread derived the same pivot
    fill_nan(false);
    if (tid == 0) info[b] = fail;
    return;
  }
  for (int o = tid; o < d * d; o += NT) wb[o] = Wm[(o / d) * ld + o % d];
  if (tid == 0) info[b] = 0;
  // y = xc W^T: a thread owns one column and 4 rows of a chunk
  const int c = tid % d, rg = tid / d;
  for (int c0 = 0; c0 < w; c0 += FCH) {
    const int nr = w - c0 < FCH ? w - c0 : FCH;
    for (int q = tid; q < nr * d4; q += NT) {
      const int r = q / d4, cc = 4 * (q % d4);
      const f32x4 v = *(const f32x4*)(xcb + (int64_t)(c0 + r) * d + cc);
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[r * ld + cc + k] = v[k];
    }
    __syncthreads();
    if (rg < FCH / 4) {
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const float* xr = xs + rg * 4 * ld;
      for (int k = 0; k <= c; ++k) {
        const double wv = (double)Wm[c * ld + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_fma((double)xr[q * ld + k], wv, acc[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (rg * 4 + q < nr) yb[(int64_t)(c0 + rg * 4 + q) * d + c] = (float)acc[q];
    }
    __syncthreads();
  }
}

template <int LDSB>
__global__ void __launch_bounds__(NT)
whiten_bwd_k(int w, int d, int n_rows, const float* __restrict__ x, const int32_t* __restrict__ rows, float eps, const float* __restrict__ mean,
             const float* __restrict__ winv, const float* __restrict__ dy, float* __restrict__ dx, float* __restrict__ xcws) {
  __shared__ __align__(16) unsigned char sm[LDSB];
  const Lay L = lds_layout(d, BCH, true);
  float* Wm = (float*)sm;
  float* B1 = (float*)(sm + L.b1);
  double* Sd = (double*)(sm + L.sd);
  float* xs = (float*)(sm + L.xs);
  float* gs = (float*)(sm + L.gs);
  float* muf = (float*)(sm + L.mu);
  double* gbd = (double*)(sm + L.gb);
  double* part = (double*)(sm + L.part);
  const int b = blockIdx.x, tid = threadIdx.x, ld = L.ld, d4 = d / 4;
  const int32_t* rb = rows + (int64_t)b * w;
  const float* gb = dy + (int64_t)b * w * d;
  float* xcb = xcws + (int64_t)b * w * d;
  if (!rows_in_range(w, n_rows, rb, (int*)(sm + L.dg))) {                  // the rows that can be named get NaN, nothing of x is read
    const float qnan = __builtin_nanf("");
    for (int o = tid; o < w * d; o += NT) {
      const int r = rb[o / d];
      if (r >= 0 && r < n_rows) dx[(int64_t)r * d + o % d] = qnan;
    }
    return;
  }
  if (tid < d) muf[tid] = mean[(int64_t)b * d + tid];
  for (int o = tid; o < d * d; o += NT) Wm[(o / d) * ld + o % d] = winv[(int64_t)b * d * d + o];
  column_means(w, d, L.P, [&](int i) { return gb + (int64_t)i * d; }, part, gbd);
  // dW = G^T xc -> B1
  auto stage = [&](int c0, int nr, bool first) {
    for (int q = tid; q < nr * d4; q += NT) {
      const int r = q / d4, c = 4 * (q % d4);
      const f32x4 g = *(const f32x4*)(gb + (int64_t)(c0 + r) * d + c);
      f32x4 o;
      if (first) {
        const f32x4 v = *(const f32x4*)(x + (int64_t)rb[c0 + r] * d + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = v[k] - muf[c + k];
        *(f32x4*)(xcb + (int64_t)(c0 + r) * d + c) = o;
      } else {
        o = *(const f32x4*)(xcb + (int64_t)(c0 + r) * d + c);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xs[r * ld + c + k] = o[k];
        gs[r * ld + c + k] = first ? g[k] : (float)((double)g[k] - gbd[c + k]);
      }
    }
    __syncthreads();
  };
  gram_dxd(w, d, ld, L.kp, BCH, gs, xs, Sd, [&](int c0, int nr) { stage(c0, nr, true); }, [&](int a, int c, double s) { B1[a * ld + c] = (float)s; });
  // Q = Phi(tril(dW W^T)):  M[i][j] = sum_{k <= j} dW[i][k] W[j][k]  (i >= j reads the lower triangle of dW only)
  inplace_dxd(B1, d, ld, [&](int a, int c) {
    if (a < c) return 0.f;
    double t = 0.0;
    for (int k = 0; k <= c; ++k) t = __builtin_fma((double)B1[a * ld + k], (double)Wm[c * ld + k], t);
    return (float)(a == c ? 0.5 * t : t);
  });
  // T1 = Q W (lower)
  inplace_dxd(B1, d, ld, [&](int a, int c) {
    if (a < c) return 0.f;
    double t = 0.0;
    for (int k = c; k <= a; ++k) t = __builtin_fma((double)B1[a * ld + k], (double)Wm[k * ld + c], t);
    return (float)t;
  });
  // T = W^T T1 (full)
  inplace_dxd(B1, d, ld, [&](int a, int c) {
    double t = 0.0;
    for (int k = a > c ? a : c; k < d; ++k) t = __builtin_fma((double)Wm[k * ld + a], (double)B1[k * ld + c], t);
    return (float)t;
  });
  // dA' = 2 (1 - eps) / (w - 1) * dA = -(1 - eps) / (w - 1) * (T + T^T)
  const double cs = -(1.0 - (double)eps) / (double)(w - 1);
  inplace_dxd(B1, d, ld, [&](int a, int c) { return (float)(cs * ((double)B1[a * ld + c] + (double)B1[c * ld + a])); });
  // dx[rows] = (G - colmean G) W + xc dA': a thread owns one column and 2 rows of a chunk
  const int c = tid % d, rg = tid / d;
  for (int c0 = 0; c0 < w; c0 += BCH) {
    const int nr = w - c0 < BCH ? w - c0 : BCH;
    stage(c0, nr, false);
    if (rg < BCH / 2) {
      double acc[2] = {0.0, 0.0};
      const float* gr = gs + rg * 2 * ld;
      const float* xr = xs + rg * 2 * ld;
      for (int k = c; k < d; ++k) {
        const double wv = (double)Wm[k * ld + c];
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q] = __builtin_fma((double)gr[q * ld + k], wv, acc[q]);
      }
      for (int k = 0; k < d; ++k) {
        const double av = (double)B1[k * ld + c];
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q] = __builtin_fma((double)xr[q * ld + k], av, acc[q]);
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (rg * 2 + q < nr) dx[(int64_t)rb[c0 + rg * 2 + q] * d + c] = (float)acc[q];
    }
    __syncthreads();
  }
}

// perm[t][0][rank of position i among the keys] = i; the key of position i is the first word of Philox(seed, step, i, PERM_VIEW_BASE + t); ties to the lower position
__global__ void __launch_bounds__(NT)
wmse_perm_k(int n, int views, uint64_t seed, uint64_t step, const int64_t* __restrict__ step_dev, int32_t* __restrict__ perm) {
  __shared__ uint32_t keys[SSV_WMSE_PERM_MAX_N];
  const int t = blockIdx.x;
  if (step_dev) step = (uint64_t)*step_dev;
  for (int i = threadIdx.x; i < n; i += NT) {
    Philox st(seed, step, (uint64_t)i, PERM_VIEW_BASE + (uint32_t)t);
    st.block();
    keys[i] = st.buf[0];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += NT) {
    const uint32_t ki = keys[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t kj = keys[j];
      rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    for (int v = 0; v < views; ++v) perm[((int64_t)t * views + v) * n + rank] = i + v * n;
  }
}

__global__ void wmse_step_advance_k(int64_t* __restrict__ step_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_dev += 1;
}

bool shape_ok(int32_t blocks, int32_t w, int32_t d) {
  return blocks >= 1 && d >= 4 && d <= MAX_D && d % 4 == 0 && w > d && w <= MAX_W && (int64_t)blocks * w < ((int64_t)1 << 31);
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool eps_ok(float eps) { return eps >= 0.f && eps < 1.f; }               // false for NaN

}  // namespace

extern "C" size_t ssv_whiten_workspace_bytes(int32_t blocks, int32_t w, int32_t d) {
  if (!shape_ok(blocks, w, d)) return 0;
  return up256((size_t)blocks * w * d * sizeof(float));                   // the centred rows, block-dense
}

#define SSV_WHITEN_LAUNCH(kernel, need, ...)                                                                                        \
  do {                                                                                                                              \
    if ((need) <= 16384) hipLaunchKernelGGL(kernel<16384>, dim3((unsigned)blocks), dim3(NT), 0, s, __VA_ARGS__);                     \
    else if ((need) <= 65536) hipLaunchKernelGGL(kernel<65536>, dim3((unsigned)blocks), dim3(NT), 0, s, __VA_ARGS__);                \
    else hipLaunchKernelGGL(kernel<163840>, dim3((unsigned)blocks), dim3(NT), 0, s, __VA_ARGS__);                                   \
  } while (0)

extern "C" int ssv_whiten_fwd(int32_t blocks, int32_t w, int32_t d, int64_t n_rows, const float* x, const int32_t* rows, float eps, float* y, float* mean,
                              float* winv, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(blocks, w, d), "ssv_whiten_fwd: need blocks >= 1, blocks * w < 2^31, d %% 4 == 0, 4 <= d <= %d, d < w <= %d (got blocks=%d w=%d d=%d)", MAX_D,
              MAX_W, blocks, w, d);
  SSV_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31), "ssv_whiten_fwd: need 1 <= n_rows < 2^31 (got %lld)", (long long)n_rows);
  SSV_REQUIRE(eps_ok(eps), "ssv_whiten_fwd: need 0 <= eps < 1 (got %g)", (double)eps);
  SSV_REQUIRE(x && rows && y && mean && winv && info && ws, "ssv_whiten_fwd: null pointer");
  SSV_REQUIRE(aligned16(x) && aligned16(rows) && aligned16(y) && aligned16(mean) && aligned16(winv) && aligned16(info) && aligned16(ws),
              "ssv_whiten_fwd: pointers must be 16-byte aligned");
  const void* in[3] = {x, rows, ws};
  const void* out[4] = {y, mean, winv, info};
  for (int a = 0; a < 4; ++a) {
    for (int b = 0; b < 3; ++b) SSV_REQUIRE(out[a] != in[b], "ssv_whiten_fwd: y, mean, winv and info alias neither each other nor an input or the workspace");
    for (int b = a + 1; b < 4; ++b) SSV_REQUIRE(out[a] != out[b], "ssv_whiten_fwd: y, mean, winv and info alias neither each other nor an input or the workspace");
  }
  const size_t need = ssv_whiten_workspace_bytes(blocks, w, d);
  SSV_REQUIRE(ws_bytes >= need, "ssv_whiten_fwd: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, s);
  const Lay L = lds_layout(d, FCH, false);
  SSV_WHITEN_LAUNCH(whiten_fwd_k, L.total, (int)w, (int)d, (int)n_rows, x, rows, eps, y, mean, winv, info, (float*)ws);
  SSV_CHECK_LAUNCH("whiten_fwd_k");
  return SSV_OK;
}

extern "C" int ssv_whiten_bwd(int32_t blocks, int32_t w, int32_t d, int64_t n_rows, const float* x, const int32_t* rows, float eps, const float* mean,
                              const float* winv, const float* dy, float* dx, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(blocks, w, d), "ssv_whiten_bwd: need blocks >= 1, blocks * w < 2^31, d %% 4 == 0, 4 <= d <= %d, d < w <= %d (got blocks=%d w=%d d=%d)", MAX_D,
              MAX_W, blocks, w, d);
  SSV_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31), "ssv_whiten_bwd: need 1 <= n_rows < 2^31 (got %lld)", (long long)n_rows);
  SSV_REQUIRE(eps_ok(eps), "ssv_whiten_bwd: need 0 <= eps < 1 (got %g)", (double)eps);
  SSV_REQUIRE(x && rows && mean && winv && dy && dx && ws, "ssv_whiten_bwd: null pointer");
  SSV_REQUIRE(aligned16(x) && aligned16(rows) && aligned16(mean) && aligned16(winv) && aligned16(dy) && aligned16(dx) && aligned16(ws),
              "ssv_whiten_bwd: pointers must be 16-byte aligned");
  const void* in[6] = {x, rows, mean, winv, dy, ws};
  for (int b = 0; b < 6; ++b) SSV_REQUIRE(dx != in[b], "ssv_whiten_bwd: dx aliases neither an input nor the workspace");
  const size_t need = ssv_whiten_workspace_bytes(blocks, w, d);
  SSV_REQUIRE(ws_bytes >= need, "ssv_whiten_bwd: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, s);
  const Lay L = lds_layout(d, BCH, true);
  SSV_WHITEN_LAUNCH(whiten_bwd_k, L.total, (int)w, (int)d, (int)n_rows, x, rows, eps, mean, winv, dy, dx, (float*)ws);
  SSV_CHECK_LAUNCH("whiten_bwd_k");
  return SSV_OK;
}

extern "C" int ssv_wmse_perm(int32_t n, int32_t views, int32_t iters, uint64_t seed, uint64_t step, int64_t* step_dev, int32_t* perm, void* stream) {
  SSV_REQUIRE(n >= 2 && n <= SSV_WMSE_PERM_MAX_N && views >= 1 && views <= SSV_WMSE_PERM_MAX_VIEWS && iters >= 1 && iters <= SSV_WMSE_PERM_MAX_ITERS,
              "ssv_wmse_perm: need 2 <= n <= %d, 1 <= views <= %d, 1 <= iters <= %d (got n=%d views=%d iters=%d)", SSV_WMSE_PERM_MAX_N, SSV_WMSE_PERM_MAX_VIEWS,
              SSV_WMSE_PERM_MAX_ITERS, n, views, iters);
  SSV_REQUIRE(perm, "ssv_wmse_perm: null pointer");
  SSV_REQUIRE(aligned16(perm) && ((uintptr_t)step_dev & 7) == 0, "ssv_wmse_perm: perm must be 16-byte aligned, step_dev 8-byte aligned");
  SSV_REQUIRE((const void*)step_dev != (const void*)perm, "ssv_wmse_perm: step_dev aliases perm");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(wmse_perm_k, dim3((unsigned)iters), dim3(NT), 0, s, (int)n, (int)views, seed, step, (const int64_t*)step_dev, perm);
  SSV_CHECK_LAUNCH("wmse_perm_k");
  if (step_dev) {
    hipLaunchKernelGGL(wmse_step_advance_k, dim3(1), dim3(64), 0, s, step_dev);
    SSV_CHECK_LAUNCH("wmse_step_advance_k");
  }
  return SSV_OK;
}
