// LARS (layer-wise adaptive rate scaling, You et al. 2017) over the flat parameter arena: the optimizer of the large-batch SimCLR / BYOL / Barlow Twins recipes.
// Per tensor t with flags decay_t, adapt_t (g2, the second view's gradient slab, may be absent):
//     u   = (g + g2) + (decay_t ? wd : 0) * p
//     q_t = eta * |p|_2 / |u|_2   if adapt_t and |p|_2 > 0 and |u|_2 > 0, else 1
//     mu  = momentum * mu + q_t * u            (mu starts at zero: no first-step flag, no Nesterov)
//     p   = p - lr * mu
// Element i needs two norms over the whole tensor it belongs to, so the step is TWO launches over the chunks of the plan (csrc/lars_plan.h), one workgroup per
// chunk of at most 8192 floats of one tensor, nothing from the host per step, no synchronisation between them but stream order:
//   lars_norms_k   chunk -> its partial sum p^2 and sum u^2: float4 loads, each thread's squares accumulated in DOUBLE (free next to the 12 bytes per element),
//                  a fixed xor tree over the wavefront, the four wavefronts added in order.  Chunks of tensors that are not adapted leave at once.
//   lars_update_k  every workgroup of a tensor folds that tensor's partials the same way - thread-strided in chunk order, then a fixed tree in LDS, in double, as
//                  kmeans_objective_k does - so all of them hold the SAME q_t bit for bit; then mu and p over the chunk.  A tensor's first chunk writes q_t.
// No floating-point atomics: equal inputs give equal bits.  lr, wd, momentum, eta come from four floats in DEVICE memory, the only form there is: the step is
// capturable into a HIP graph as it stands (ssv_sgd_nesterov_dev).  u is the same fused multiply-add in both kernels.
// Bytes per parameter with two slabs: 12 read by the norms pass (p, g, g2), 24 by the update (p, g, g2, mu read; mu, p written) - 36 against the 24 of ssv_sgd_nesterov.
// Padding floats between tensors belong to no chunk.  A record of the plan that points outside the arena or the tables is skipped, never followed.
#include "common.h"
#include "lars_plan.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool TWO>
__device__ __forceinline__ f32x4 lars_u4(const float* __restrict__ g, const float* __restrict__ g2, int64_t i4, const f32x4& pv, float wd) {
  f32x4 gv = reinterpret_cast<const f32x4*>(g)[i4];
  if constexpr (TWO) gv += reinterpret_cast<const f32x4*>(g2)[i4];              // view-0 slab + view-1 slab, fixed order
  f32x4 u;
#pragma unroll
  for (int e = 0; e < 4; ++e) u[e] = __builtin_fmaf(wd, pv[e], gv[e]);
  return u;
}
template <bool TWO>
__device__ __forceinline__ float lars_u1(const float* __restrict__ g, const float* __restrict__ g2, int64_t i, float pv, float wd) {
  return __builtin_fmaf(wd, pv, TWO ? g[i] + g2[i] : g[i]);
}

// what both kernels check of their chunk before they follow it
__device__ __forceinline__ bool chunk_ok(const LarsChunk& c, int64_t n, int T) {
  return (unsigned)c.tensor < (unsigned)T && c.len >= 1 && c.len <= LARS_CHUNK_FLOATS && c.start >= 0 && (c.start & 3) == 0 && c.start <= n - c.len;
}

template <bool TWO>
__global__ void __launch_bounds__(256)
lars_norms_k(int64_t n, int T, const LarsChunk* __restrict__ chunks, const LarsTensor* __restrict__ tensors, const float* __restrict__ p,
             const float* __restrict__ g, const float* __restrict__ g2, const float* __restrict__ hyper, double* __restrict__ partial) {
  __shared__ double sw[4][2];
  const LarsChunk c = chunks[blockIdx.x];
  const int flags = chunk_ok(c, n, T) ? tensors[c.tensor].flags : 0;
  if (!(flags & LARS_ADAPT)) {                                                    // q_t = 1 whatever the norms: nothing to read
    if (threadIdx.x == 0) { partial[2 * (int64_t)blockIdx.x] = 0.0; partial[2 * (int64_t)blockIdx.x + 1] = 0.0; }
    return;
  }
  const float wd = (flags & LARS_DECAY) ? hyper[1] : 0.f;
  const int len4 = c.len >> 2;
  const int64_t s4 = c.start >> 2;
  double sp = 0.0, su = 0.0;
  for (int i = threadIdx.x; i < len4; i += 256) {
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[s4 + i];
    const f32x4 u = lars_u4<TWO>(g, g2, s4 + i, pv, wd);
#pragma unroll
    for (int e = 0; e < 4; ++e) { sp = __builtin_fma((double)pv[e], (double)pv[e], sp); su = __builtin_fma((double)u[e], (double)u[e], su); }
  }
  for (int i = (len4 << 2) + threadIdx.x; i < c.len; i += 256) {                  // the last chunk of a tensor: up to 3 floats behind its float4s
    const float pv = p[c.start + i];
    const float u = lars_u1<TWO>(g, g2, c.start + i, pv, wd);
    sp = __builtin_fma((double)pv, (double)pv, sp);
    su = __builtin_fma((double)u, (double)u, su);
  }
  sp = wave_sum_f64(sp);
  su = wave_sum_f64(su);
  if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = sp; sw[threadIdx.x >> 6][1] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * (int64_t)blockIdx.x] = ((sw[0][0] + sw[1][0]) + sw[2][0]) + sw[3][0];
    partial[2 * (int64_t)blockIdx.x + 1] = ((sw[0][1] + sw[1][1]) + sw[2][1]) + sw[3][1];
  }
}

template <bool TWO>
__global__ void __launch_bounds__(256)
lars_update_k(int64_t n, int T, int nchunks, const LarsChunk* __restrict__ chunks, const LarsTensor* __restrict__ tensors, float* __restrict__ p,
              const float* __restrict__ g, const float* __restrict__ g2, float* __restrict__ mu, const float* __restrict__ hyper,
              const double* __restrict__ partial, float* __restrict__ ratios) {
  __shared__ double sm[2][256];
  __shared__ float qs;
  const LarsChunk c = chunks[blockIdx.x];
  if (!chunk_ok(c, n, T)) return;
  const LarsTensor t = tensors[c.tensor];
  const float lr = hyper[0], wd = (t.flags & LARS_DECAY) ? hyper[1] : 0.f, mom = hyper[2], eta = hyper[3];
  float q = 1.f;
  if ((t.flags & LARS_ADAPT) && t.first >= 0 && t.count >= 1 && t.first <= nchunks - t.count) {     // uniform over the workgroup
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < t.count; i += 256) { a += partial[2 * (int64_t)(t.first + i)]; b += partial[2 * (int64_t)(t.first + i) + 1]; }
    sm[0][threadIdx.x] = a;
    sm[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) { sm[0][threadIdx.x] += sm[0][threadIdx.x + o]; sm[1][threadIdx.x] += sm[1][threadIdx.x + o]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double sp = sm[0][0], su = sm[1][0];
      qs = (sp > 0.0 && su > 0.0) ? (float)((double)eta * sqrt(sp) / sqrt(su)) : 1.f;               // a NaN norm compares false: q = 1, and the NaN reaches p through u
    }
    __syncthreads();
    q = qs;
  }
  if (threadIdx.x == 0 && (int)blockIdx.x == t.first) ratios[c.tensor] = q;
  const int len4 = c.len >> 2;
  const int64_t s4 = c.start >> 2;
  for (int i = threadIdx.x; i < len4; i += 256) {
    const f32x4 pv = reinterpret_cast<f32x4*>(p)[s4 + i];
    const f32x4 u = lars_u4<TWO>(g, g2, s4 + i, pv, wd);
    const f32x4 mv = reinterpret_cast<f32x4*>(mu)[s4 + i];
    f32x4 mn, pn;
#pragma unroll
    for (int e = 0; e < 4; ++e) { mn[e] = __builtin_fmaf(mom, mv[e], q * u[e]); pn[e] = __builtin_fmaf(-lr, mn[e], pv[e]); }
    reinterpret_cast<f32x4*>(mu)[s4 + i] = mn;
    reinterpret_cast<f32x4*>(p)[s4 + i] = pn;
  }
  for (int i = (len4 << 2) + threadIdx.x; i < c.len; i += 256) {
    const float pv = p[c.start + i];
    const float u = lars_u1<TWO>(g, g2, c.start + i, pv, wd);
    const float mn = __builtin_fmaf(mom, mu[c.start + i], q * u);
    mu[c.start + i] = mn;
    p[c.start + i] = __builtin_fmaf(-lr, mn, pv);
  }
}

}  // namespace

extern "C" int64_t ssv_lars_chunk_floats(void) { return LARS_CHUNK_FLOATS; }

extern "C" int64_t ssv_lars_plan_chunks(int32_t T, const int64_t* numel) { return lars_plan_chunks(T, numel); }

extern "C" size_t ssv_lars_plan_bytes(int32_t T, const int64_t* numel) { return lars_plan_bytes(T, numel); }

extern "C" int ssv_lars_plan_build(int32_t T, const int64_t* offset, const int64_t* numel, const int32_t* decay, const int32_t* adapt, void* plan, size_t plan_bytes) {
  char why[256] = "lars plan: refused";
  const int rc = lars_plan_build(T, offset, numel, decay, adapt, plan, plan_bytes, why, sizeof(why));
  if (rc != SSV_OK) SSV_FAIL(rc, "ssv_lars_plan_build: %s", why);
  return SSV_OK;
}

extern "C" size_t ssv_lars_workspace_bytes(int64_t nchunks) { return nchunks >= 1 && nchunks <= INT32_MAX ? (size_t)nchunks * 2 * sizeof(double) : 0; }

extern "C" int ssv_lars_step(int64_t n, int32_t T, int64_t nchunks, const void* plan, float* p, const float* g, const float* g2, float* mu,
                             const float* hyper, float* ratios, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(n > 0 && n <= LARS_MAX_ARENA && T >= 1 && nchunks >= T && nchunks <= INT32_MAX,
              "ssv_lars_step: need n >= 1, T >= 1 and T <= nchunks < 2^31 (got n=%lld T=%d nchunks=%lld)", (long long)n, T, (long long)nchunks);
  SSV_REQUIRE(plan && p && g && mu && hyper && ratios && ws, "ssv_lars_step: null pointer");
  SSV_REQUIRE((((uintptr_t)plan | (uintptr_t)p | (uintptr_t)g | (uintptr_t)g2 | (uintptr_t)mu | (uintptr_t)hyper | (uintptr_t)ws) & 15) == 0,
              "ssv_lars_step: pointers must be 16-byte aligned");
  const size_t need = ssv_lars_workspace_bytes(nchunks);
  if (ws_bytes < need) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_lars_step: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_OPTIM, s);
  const LarsChunk* chunks = (const LarsChunk*)plan;
  const LarsTensor* tensors = (const LarsTensor*)((const char*)plan + (size_t)nchunks * sizeof(LarsChunk));
  double* partial = (double*)ws;
  const dim3 grid((unsigned)nchunks), block(256);
  if (g2) hipLaunchKernelGGL((lars_norms_k<true>), grid, block, 0, s, n, (int)T, chunks, tensors, (const float*)p, g, g2, hyper, partial);
  else    hipLaunchKernelGGL((lars_norms_k<false>), grid, block, 0, s, n, (int)T, chunks, tensors, (const float*)p, g, g2, hyper, partial);
  SSV_CHECK_LAUNCH("lars_norms_k");
  if (g2) hipLaunchKernelGGL((lars_update_k<true>), grid, block, 0, s, n, (int)T, (int)nchunks, chunks, tensors, p, g, g2, mu, hyper, (const double*)partial, ratios);
  else    hipLaunchKernelGGL((lars_update_k<false>), grid, block, 0, s, n, (int)T, (int)nchunks, chunks, tensors, p, g, g2, mu, hyper, (const double*)partial, ratios);
  SSV_CHECK_LAUNCH("lars_update_k");
  return SSV_OK;
}
