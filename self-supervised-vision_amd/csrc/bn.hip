// Training-mode BatchNorm over the rows of an [M][C] fp32 matrix (NHWC activations: M = N*H*W),
// fused with ReLU and the residual add, plus the column-sum used for Linear bias gradients.
// All of it is HBM-streaming work: float4 per lane along C (coalesced rows), every thread keeps
// its channel group fixed and walks rows, per-block partials are merged in a FIXED order
// (deterministic) with double precision in the finalize kernels.
//
// Statistics: per block shifted sums  S1 = sum(x-K), S2 = sum((x-K)^2)  with K = first row of the
// block (kills the E[x^2]-E[x]^2 cancellation), turned into (mean_b, M2_b) and merged with Chan's
// formula in double - the same accumulation width ATen's CPU batch_norm uses (acc_type<float> = double).
#include "common.h"
#include "bn_plan.h"
#include "row_stream.h"

namespace {

// ---- forward statistics ----------------------------------------------------------------------
__global__ void __launch_bounds__(256)
bn_stats_k(int64_t M, int C, int CT, int RT, int rpb, const float* __restrict__ x, float* __restrict__ pmean, float* __restrict__ pm2) {
  __shared__ f32x4 sm1[256], sm2[256];
  SSV_ROW_LANE(M, C, CT, RT, rpb);
  f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0}, K = {0, 0, 0, 0};
  if (active) {
    K = ld4(x + r0 * C + 4 * c4);
    int64_t r = r0 + rt;
    for (; r + 3 * RT < r1; r += 4 * RT) {          // 4 independent 16-B loads in flight per lane; the paired summation is part of the result
      const f32x4 v0 = ld4(x + r * C + 4 * c4) - K, v1 = ld4(x + (r + RT) * C + 4 * c4) - K;
      const f32x4 v2 = ld4(x + (r + 2 * RT) * C + 4 * c4) - K, v3 = ld4(x + (r + 3 * RT) * C + 4 * c4) - K;
      s1 += (v0 + v1) + (v2 + v3); s2 += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
    }
    for (; r < r1; r += RT) {
      const f32x4 v = ld4(x + r * C + 4 * c4) - K;
      s1 += v; s2 += v * v;
    }
  }
  SSV_BLOCK_TAIL2(CT, RT, sm1, sm2, s1, s2,
    const float n = (float)(r1 - r0);
    const f32x4 mean = K + s1 / n, m2 = s2 - s1 * s1 / n;
    st_partial(pmean, c4, C, mean); st_partial(pm2, c4, C, m2););
}

// Merge of the per-block (mean_b, M2_b): FIN_C channels x FIN_G groups of partial blocks per workgroup (row_stream.h); two
// division-free passes in double, fixed summation order:
//   mean = sum_b n_b*mean_b / M ;  M2 = sum_b (M2_b + n_b*(mean_b-mean)^2)
__global__ void __launch_bounds__(256)
bn_stats_finalize_k(int64_t M, int C, int rpb, int nblk, const float* __restrict__ pmean, const float* __restrict__ pm2,
                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                    float* running_mean, float* running_var, int64_t* nbt,
                    float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double sm[FIN_G][FIN_C];
  const FinLane f = fin_lane(C, nblk);
  const int c = f.c;
  const double last_n = (double)(M - (int64_t)(nblk - 1) * rpb), full_n = (double)rpb;
  double acc = 0.0;
  if (f.ok) acc = fin_group_sum(f.b0, f.b1, [&](int b) { return (b == nblk - 1 ? last_n : full_n) * (double)pmean[(size_t)b * C + c]; });
  fin_put(sm, f, acc);
  __syncthreads();
  const double mean = fin_sum(sm, f) / (double)M;
  __syncthreads();
  acc = 0.0;
  if (f.ok) acc = fin_group_sum(f.b0, f.b1, [&](int b) {
    const double d = (double)pmean[(size_t)b * C + c] - mean;
    return (double)pm2[(size_t)b * C + c] + (b == nblk - 1 ? last_n : full_n) * d * d; });
  fin_put(sm, f, acc);
  __syncthreads();
  if (f.grp == 0 && f.ok) {
    const double m2 = fin_sum(sm, f);
    const double var = m2 / (double)M;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float fmean = (float)mean;
    save_mean[c] = fmean;
    save_invstd[c] = invstd;
    const float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - fmean * sc;
    if (running_mean) {
      const float unbiased = (float)(M > 1 ? m2 / (double)(M - 1) : var);
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * fmean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
    }
    if (nbt && c == 0) *nbt += 1;
  }
}

// With RELU the kernel can also write the ReLU mask, one byte per float4 (bit e = element e was positive): the backward
// then reads 1 byte instead of the 16 bytes of y for each group of four elements.
// RES: 0 none, 1 add a materialised residual, 2 add a residual that is itself a BatchNorm of a raw conv output
// (res * rscale + rshift: the projection shortcut's BatchNorm folded into the block's closing kernel)
template <bool RELU, int RES>
__global__ void __launch_bounds__(256)
bn_apply_k(int64_t M, int C, int CT, int RT, int rpb, const float* __restrict__ x, const float* __restrict__ scale,
           const float* __restrict__ shift, const float* __restrict__ res, const float* __restrict__ rscale, const float* __restrict__ rshift,
           float* __restrict__ y, uint8_t* __restrict__ mask) {
  SSV_ROW_LANE_OR_RETURN(M, C, CT, RT, rpb);
  const f32x4 sc = ld4(scale + 4 * c4), sh = ld4(shift + 4 * c4);
  f32x4 rsc = {0, 0, 0, 0}, rsh = {0, 0, 0, 0};
  if constexpr (RES == 2) { rsc = ld4(rscale + 4 * c4); rsh = ld4(rshift + 4 * c4); }
  auto body = [&](int64_t r) {
    const size_t o = (size_t)r * C + 4 * c4;
    f32x4 v = fma4(ld4(x + o), sc, sh);
    if constexpr (RES == 1) v += ld4(res + o);
    if constexpr (RES == 2) v += fma4(ld4(res + o), rsc, rsh);
    if constexpr (RELU) {
      if (mask) mask[o >> 2] = (uint8_t)((v[0] > 0.f) | ((v[1] > 0.f) << 1) | ((v[2] > 0.f) << 2) | ((v[3] > 0.f) << 3));
      v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
    }
    st4(y + o, v);
  };
  SSV_WALK4(r0 + rt, r1, RT, body);
}

// ---- backward ----------------------------------------------------------------------------------
template <bool RELU>
__device__ __forceinline__ f32x4 masked(f32x4 g, f32x4 yv) {
  if constexpr (RELU) {
    g[0] = yv[0] > 0.f ? g[0] : 0.f; g[1] = yv[1] > 0.f ? g[1] : 0.f;
    g[2] = yv[2] > 0.f ? g[2] : 0.f; g[3] = yv[3] > 0.f ? g[3] : 0.f;
  }
  return g;
}
// g masked by ReLU: from the byte mask when the forward wrote one, else from the sign of y
__device__ __forceinline__ f32x4 relu_grad(f32x4 g, const float* __restrict__ y, const uint8_t* __restrict__ mask, size_t o) {
  if (mask) {
    const unsigned b = mask[o >> 2];
    g[0] = (b & 1u) ? g[0] : 0.f; g[1] = (b & 2u) ? g[1] : 0.f; g[2] = (b & 4u) ? g[2] : 0.f; g[3] = (b & 8u) ? g[3] : 0.f;
    return g;
  }
  return masked<true>(g, ld4(y + o));
}

// RELU: 0 no ReLU behind this BatchNorm, 1 mask from the byte mask / the sign of y, 2 mask recomputed as x * scale + shift > 0
// (the fused path never materialises y nor a mask for conv -> BN -> ReLU -> conv chains; scale / shift are the forward's own
// floats, so the recomputed mask is the forward's ReLU bit for bit)
template <int RELU>
__device__ __forceinline__ f32x4 bwd_gate(f32x4 g, f32x4 xv, f32x4 sc, f32x4 sh, const float* __restrict__ y, const uint8_t* __restrict__ mask, size_t o) {
  if constexpr (RELU == 1) return relu_grad(g, y, mask, o);
  if constexpr (RELU == 2) return masked<true>(g, fma4(xv, sc, sh));
  return g;
}

template <int RELU>
__global__ void __launch_bounds__(256)
bn_bwd_reduce_k(int64_t M, int C, int CT, int RT, int rpb, const float* __restrict__ dy, const float* __restrict__ y,
                const uint8_t* __restrict__ mask, const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ psg, float* __restrict__ psgx) {
  __shared__ f32x4 sm1[256], sm2[256];
  SSV_ROW_LANE(M, C, CT, RT, rpb);
  f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
  if (active) {
    const f32x4 mu = ld4(mean + 4 * c4), is = ld4(invstd + 4 * c4);
    f32x4 sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
    if constexpr (RELU == 2) { sc = ld4(scale + 4 * c4); sh = ld4(shift + 4 * c4); }
    auto body = [&](int64_t r) {
      const size_t o = (size_t)r * C + 4 * c4;
      const f32x4 xv = ld4(x + o);
      bn_bwd_acc(bwd_gate<RELU>(ld4(dy + o), xv, sc, sh, y, mask, o), xv, mu, is, s1, s2);
    };
    SSV_WALK4(r0 + rt, r1, RT, body);
  }
  SSV_BLOCK_TAIL2(CT, RT, sm1, sm2, s1, s2, st_partial(psg, c4, C, s1); st_partial(psgx, c4, C, s2););
}

__global__ void __launch_bounds__(256)
bn_bwd_finalize_k(int64_t M, int C, int nblk, const float* __restrict__ psg, const float* __restrict__ psgx,
                  float* dgamma, float* dbeta, int accumulate, float* __restrict__ k1, float* __restrict__ k2,
                  const float* __restrict__ gamma = nullptr, const float* __restrict__ mean = nullptr, const float* __restrict__ invstd = nullptr,
                  float* __restrict__ coef = nullptr) {
  __shared__ double s1[FIN_G][FIN_C], s2[FIN_G][FIN_C];
  const FinLane f = fin_lane(C, nblk);
  const int c = f.c;
  double sg = 0.0, sgx = 0.0;
  if (f.ok) {
    sg = fin_group_sum(f.b0, f.b1, [&](int b) { return (double)psg[(size_t)b * C + c]; });
    sgx = fin_group_sum(f.b0, f.b1, [&](int b) { return (double)psgx[(size_t)b * C + c]; });
  }
  fin_put(s1, f, sg); fin_put(s2, f, sgx);
  __syncthreads();
  if (f.grp == 0 && f.ok) {
    fin_sum(s1, s2, f, sg, sgx);
    if (k1) { k1[c] = (float)(sg / (double)M); k2[c] = (float)(sgx / (double)M); }
    if (coef) {      // dx = A * g + B * (x - mean) + D  (ssv_bn_dyin: the consumer convolutions form dx while they stage it)
      const double gi = (double)gamma[c] * (double)invstd[c];
      coef[c] = (float)gi;
      coef[C + c] = mean[c];
      coef[2 * C + c] = (float)(-gi * (double)invstd[c] * (sgx / (double)M));
      coef[3 * C + c] = (float)(-gi * (sg / (double)M));
    }
    if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)sgx;
    if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)sg;
  }
}

template <int RELU, bool DRES>
__global__ void __launch_bounds__(256)
bn_bwd_apply_k(int64_t M, int C, int CT, int RT, int rpb, const float* __restrict__ dy, const float* __restrict__ y,
               const uint8_t* __restrict__ mask, const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ mean,
               const float* __restrict__ invstd, const float* __restrict__ scale, const float* __restrict__ shift,
               const float* __restrict__ k1, const float* __restrict__ k2, float* __restrict__ dx, float* __restrict__ dres) {
  SSV_ROW_LANE_OR_RETURN(M, C, CT, RT, rpb);
  const f32x4 mu = ld4(mean + 4 * c4), is = ld4(invstd + 4 * c4);
  const f32x4 gi = ld4(gamma + 4 * c4) * is, a1 = ld4(k1 + 4 * c4), a2 = ld4(k2 + 4 * c4);
  f32x4 sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
  if constexpr (RELU == 2) { sc = ld4(scale + 4 * c4); sh = ld4(shift + 4 * c4); }
  auto body = [&](int64_t r) {
    const size_t o = (size_t)r * C + 4 * c4;
    const f32x4 xv = ld4(x + o);
    const f32x4 g = bwd_gate<RELU>(ld4(dy + o), xv, sc, sh, y, mask, o);
    bn_bwd_dx(dx + o, g, xv, mu, is, gi, a1, a2);
    if constexpr (DRES) st4(dres + o, g);
  };
  SSV_WALK4(r0 + rt, r1, RT, body);
}

// ---- column sum --------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
colsum_partial_k(int64_t M, int C, int CT, int RT, int rpb, const float* __restrict__ x, float* __restrict__ ps) {
  __shared__ f32x4 sm1[256];
  SSV_ROW_LANE(M, C, CT, RT, rpb);
  f32x4 s1 = {0, 0, 0, 0};
  if (active) for (int64_t r = r0 + rt; r < r1; r += RT) s1 += ld4(x + (size_t)r * C + 4 * c4);
  SSV_BLOCK_TAIL(CT, RT, sm1, s1, st_partial(ps, c4, C, s1););
}
__global__ void __launch_bounds__(256)
colsum_finalize_k(int C, int nblk, const float* __restrict__ ps, float* out, int accumulate) {
  __shared__ double s1[FIN_G][FIN_C];
  const FinLane f = fin_lane(C, nblk);
  const int c = f.c;
  double s = 0.0;
  if (f.ok) s = fin_group_sum(f.b0, f.b1, [&](int b) { return (double)ps[(size_t)b * C + c]; });
  fin_put(s1, f, s);
  __syncthreads();
  if (f.grp == 0 && f.ok) {
    s = fin_sum(s1, f);
    out[c] = (accumulate ? out[c] : 0.f) + (float)s;
  }
}

int check_mc(int64_t M, int C, const char* who) {
  SSV_REQUIRE(M > 0 && C > 0 && C % 4 == 0, "%s: need M > 0, C > 0, C %% 4 == 0 (M=%lld C=%d)", who, (long long)M, C);
  SSV_REQUIRE(M < (1ll << 31), "%s: M too large", who);
  return SSV_OK;
}

// Merge `factor` consecutive fine partials (rows-per-block rpb, the last one ragged) into one coarse partial per channel, in double
// and in fixed order, so that the finalize kernel walks M / (rpb * factor) partials instead of M / rpb.
__global__ void __launch_bounds__(256)
bn_partials_coarsen_k(int64_t M, int C, int rpb, int nblk, int factor, const float* __restrict__ pmean, const float* __restrict__ pm2,
                      float* __restrict__ cmean, float* __restrict__ cm2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (c >= C) return;
  const int b0 = j * factor, b1 = min(b0 + factor, nblk);
  const double last_n = (double)(M - (int64_t)(nblk - 1) * rpb), full_n = (double)rpb;
  double tot = 0.0, sum = 0.0;
  for (int b = b0; b < b1; ++b) { const double n = b == nblk - 1 ? last_n : full_n; tot += n; sum += n * (double)pmean[(size_t)b * C + c]; }
  const double mean = sum / tot;
  double m2 = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double n = b == nblk - 1 ? last_n : full_n, d = (double)pmean[(size_t)b * C + c] - mean;
    m2 += (double)pm2[(size_t)b * C + c] + n * d * d;
  }
  cmean[(size_t)j * C + c] = (float)mean;
  cm2[(size_t)j * C + c] = (float)m2;
}

// partial sums of the backward: plain sums, same two-level scheme
__global__ void __launch_bounds__(256)
bn_sums_coarsen_k(int C, int nblk, int factor, const float* __restrict__ p1, const float* __restrict__ p2, float* __restrict__ c1, float* __restrict__ c2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (c >= C) return;
  const int b0 = j * factor, b1 = min(b0 + factor, nblk);
  double a = 0.0, b_ = 0.0;
  for (int b = b0; b < b1; ++b) { a += (double)p1[(size_t)b * C + c]; b_ += (double)p2[(size_t)b * C + c]; }
  c1[(size_t)j * C + c] = (float)a;
  c2[(size_t)j * C + c] = (float)b_;
}

void launch_apply(const BnPlan& p, int64_t M, int C, const float* x, const float* scale, const float* shift, const float* res,
                  const float* rscale, const float* rshift, int relu, float* y, uint8_t* mask, hipStream_t s) {
  const ApplyGrid ag = apply_grid(p, M);
  const dim3 grid(ag.nblk, p.GY);
  const int mode = res ? (rscale ? 2 : 1) : 0;
#define APPLY(R_, M_) hipLaunchKernelGGL((bn_apply_k<R_, M_>), grid, dim3(256), 0, s, M, C, p.CT, p.RT, ag.rpb, x, scale, shift, res, rscale, rshift, y, mask)
  if (relu) { if (mode == 2) APPLY(true, 2); else if (mode == 1) APPLY(true, 1); else APPLY(true, 0); }
  else      { if (mode == 2) APPLY(false, 2); else if (mode == 1) APPLY(false, 1); else APPLY(false, 0); }
#undef APPLY
}

// The two-level merge (bn_plan.h: merge_plan), one helper each way: more than 2048 partials are first coarsened into `coarse` (room for coarse_floats), and the
// caller's pointers, count (and rows per partial) then name the coarse ones.
int coarsen_stats(int64_t M, int C, const float*& pmean, const float*& pm2, int& rpb, int& nblk, float* coarse, size_t coarse_floats, hipStream_t s) {
  const MergePlan mp = merge_plan(nblk, (int64_t)(coarse_floats / ((size_t)2 * C)));
  if (!mp.factor) return SSV_OK;
  SSV_REQUIRE((size_t)2 * mp.ncoarse * C <= coarse_floats, "bn finalize: workspace too small for the coarse partials");
  float* cm2 = coarse + (size_t)mp.ncoarse * C;
  hipLaunchKernelGGL(bn_partials_coarsen_k, dim3(cdiv(C, 256), mp.ncoarse), dim3(256), 0, s, M, C, rpb, nblk, mp.factor, pmean, pm2, coarse, cm2);
  pmean = coarse; pm2 = cm2; rpb *= mp.factor; nblk = mp.ncoarse;
  return SSV_OK;
}
int coarsen_sums(int C, const float*& p1, const float*& p2, int& nblk, float* coarse, size_t coarse_floats, hipStream_t s) {
  const MergePlan mp = merge_plan(nblk, (int64_t)(coarse_floats / ((size_t)2 * C)));
  if (!mp.factor) return SSV_OK;
  SSV_REQUIRE((size_t)2 * mp.ncoarse * C <= coarse_floats, "bn backward: workspace too small for the coarse partials");
  float* c2 = coarse + (size_t)mp.ncoarse * C;
  hipLaunchKernelGGL(bn_sums_coarsen_k, dim3(cdiv(C, 256), mp.ncoarse), dim3(256), 0, s, C, nblk, mp.factor, p1, p2, coarse, c2);
  p1 = coarse; p2 = c2; nblk = mp.ncoarse;
  return SSV_OK;
}

// statistics partials (rows_per_group rows each, the last ragged) -> mean / invstd / scale / shift (+ running statistics)
int launch_finalize(int64_t M, int C, const float* pmean, const float* pm2, int rpb, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, int64_t* nbt, float* save_mean, float* save_invstd, float* scale, float* shift,
                    float* coarse, size_t coarse_floats, hipStream_t s) {
  int nblk = (int)cdiv64(M, rpb);
  if (int rc = coarsen_stats(M, C, pmean, pm2, rpb, nblk, coarse, coarse_floats, s)) return rc;
  hipLaunchKernelGGL(bn_stats_finalize_k, dim3(cdiv(C, FIN_C)), dim3(256), 0, s, M, C, rpb, nblk, pmean, pm2,
                     gamma, beta, eps, momentum, running_mean, running_var, nbt, save_mean, save_invstd, scale, shift);
  return SSV_OK;
}
}  // namespace

extern "C" size_t ssv_bn_workspace_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C % 4) return 0;
  return bn_ws_floats(bn_plan(M, C), C) * sizeof(float);
}

extern "C" int ssv_bn_train_fwd(int64_t M, int32_t C, const float* x, const float* gamma, const float* beta,
                                const float* residual, int relu, float eps, float momentum,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float* y, uint8_t* relu_mask, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_train_fwd")) return rc;
  SSV_REQUIRE(x && gamma && beta && y && save_mean && save_invstd && ws, "ssv_bn_train_fwd: null pointer");
  SSV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "ssv_bn_train_fwd: running_mean/var must both be given or both NULL");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_train_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_FWD, s);
  const BnPlan p = bn_plan(M, C);
  const BnWs w = ws_partials_first(ws, p, C);                 // pmean | pm2 | scale | shift
  hipLaunchKernelGGL(bn_stats_k, dim3(p.nblk, p.GY), dim3(256), 0, s, M, C, p.CT, p.RT, p.rpb, x, w.a, w.b);
  hipLaunchKernelGGL(bn_stats_finalize_k, dim3(cdiv(C, FIN_C)), dim3(256), 0, s, M, C, p.rpb, p.nblk, (const float*)w.a, (const float*)w.b,
                     gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, w.u, w.v);
  launch_apply(p, M, C, x, w.u, w.v, residual, nullptr, nullptr, relu, y, relu_mask, s);
  SSV_CHECK_LAUNCH("ssv_bn_train_fwd");
  return SSV_OK;
}

// Same as ssv_bn_train_fwd, but the statistics partials come from the producer (ssv_conv2d_fwd_stats): no pass over x for them.
extern "C" int ssv_bn_train_fwd_partials(int64_t M, int32_t C, const float* x, const float* pmean, const float* pm2, int32_t rows_per_group,
                                         const float* gamma, const float* beta, const float* residual, int relu, float eps, float momentum,
                                         float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                         float* y, uint8_t* relu_mask, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_train_fwd_partials")) return rc;
  SSV_REQUIRE(x && pmean && pm2 && rows_per_group > 0 && gamma && beta && y && save_mean && save_invstd && ws, "ssv_bn_train_fwd_partials: bad arguments");
  SSV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "ssv_bn_train_fwd_partials: running_mean/var must both be given or both NULL");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_train_fwd_partials: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_FWD, s);
  const BnPlan p = bn_plan(M, C);
  const BnWs w = ws_vectors_first(ws, C);                     // scale | shift | coarse partials
  if (int rc = launch_finalize(M, C, pmean, pm2, rows_per_group, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked,
                               save_mean, save_invstd, w.u, w.v, w.a, bn_coarse_floats(p, C), s)) return rc;
  launch_apply(p, M, C, x, w.u, w.v, residual, nullptr, nullptr, relu, y, relu_mask, s);
  SSV_CHECK_LAUNCH("ssv_bn_train_fwd_partials");
  return SSV_OK;
}

// ---- the fused path's pieces: statistics -> affine, and the apply on its own ---------------------------------------------------
extern "C" int ssv_bn_stats_finalize(int64_t M, int32_t C, const float* pmean, const float* pm2, int32_t rows_per_group,
                                     const float* gamma, const float* beta, float eps, float momentum,
                                     float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                     float* save_mean, float* save_invstd, float* scale, float* shift, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_stats_finalize")) return rc;
  SSV_REQUIRE(pmean && pm2 && rows_per_group > 0 && gamma && beta && save_mean && save_invstd && scale && shift && ws, "ssv_bn_stats_finalize: bad arguments");
  SSV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "ssv_bn_stats_finalize: running_mean/var must both be given or both NULL");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_stats_finalize: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_FWD, s);
  if (int rc = launch_finalize(M, C, pmean, pm2, rows_per_group, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked,
                               save_mean, save_invstd, scale, shift, (float*)ws, bn_coarse_floats(bn_plan(M, C), C), s)) return rc;   // scale / shift are the caller's: the coarse partials lead
  SSV_CHECK_LAUNCH("ssv_bn_stats_finalize");
  return SSV_OK;
}

extern "C" int ssv_bn_apply(int64_t M, int32_t C, const float* x, const float* scale, const float* shift,
                            const float* residual, const float* res_scale, const float* res_shift, int relu,
                            float* y, uint8_t* relu_mask, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_apply")) return rc;
  SSV_REQUIRE(x && scale && shift && y, "ssv_bn_apply: null pointer");
  SSV_REQUIRE((res_scale == nullptr) == (res_shift == nullptr) && (!res_scale || residual), "ssv_bn_apply: res_scale / res_shift go together and need a residual");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_FWD, s);
  launch_apply(bn_plan(M, C), M, C, x, scale, shift, residual, res_scale, res_shift, relu, y, relu_mask, s);
  SSV_CHECK_LAUNCH("ssv_bn_apply");
  return SSV_OK;
}

namespace {
void launch_bwd_finalize(int64_t M, int C, int nblk, const float* psg, const float* psgx, float* dgamma, float* dbeta, int accumulate, float* k1, float* k2,
                         hipStream_t s, const float* gamma = nullptr, const float* mean = nullptr, const float* invstd = nullptr, float* coef = nullptr) {
  hipLaunchKernelGGL(bn_bwd_finalize_k, dim3(cdiv(C, FIN_C)), dim3(256), 0, s, M, C, nblk, psg, psgx, dgamma, dbeta, accumulate, k1, k2, gamma, mean, invstd, coef);
}

// relu_mode: 0 none, 1 byte mask / sign of y, 2 recomputed from x * scale + shift
void launch_bwd_apply(const BnPlan& p, int64_t M, int C, const float* dy, const float* y, const uint8_t* relu_mask, const float* x, const float* gamma,
                      const float* save_mean, const float* save_invstd, const float* scale, const float* shift, int relu_mode,
                      const float* k1, const float* k2, float* dx, float* dresidual, hipStream_t s) {
  const ApplyGrid ag = apply_grid(p, M);
  const dim3 agrid(ag.nblk, p.GY);
#define BAPPLY(R_, D_) hipLaunchKernelGGL((bn_bwd_apply_k<R_, D_>), agrid, dim3(256), 0, s, M, C, p.CT, p.RT, ag.rpb, dy, y, relu_mask, x, gamma, save_mean, save_invstd, scale, shift, k1, k2, dx, dresidual)
  if (dresidual) { if (relu_mode == 2) BAPPLY(2, true); else if (relu_mode == 1) BAPPLY(1, true); else BAPPLY(0, true); }
  else           { if (relu_mode == 2) BAPPLY(2, false); else if (relu_mode == 1) BAPPLY(1, false); else BAPPLY(0, false); }
#undef BAPPLY
}

void launch_bwd(int64_t M, int C, const float* dy, const float* y, const uint8_t* relu_mask, const float* x, const float* gamma,
                const float* save_mean, const float* save_invstd, const float* scale, const float* shift, int relu_mode,
                float* dx, float* dresidual, float* dgamma, float* dbeta, int accumulate, void* ws, hipStream_t s) {
  const BnPlan p = bn_plan(M, C);
  const BnWs w = ws_partials_first(ws, p, C);                 // psg | psgx | k1 | k2
  const dim3 grid(p.nblk, p.GY);
#define REDUCE(R_) hipLaunchKernelGGL((bn_bwd_reduce_k<R_>), grid, dim3(256), 0, s, M, C, p.CT, p.RT, p.rpb, dy, y, relu_mask, x, save_mean, save_invstd, scale, shift, w.a, w.b)
  if (relu_mode == 2) REDUCE(2); else if (relu_mode == 1) REDUCE(1); else REDUCE(0);
#undef REDUCE
  launch_bwd_finalize(M, C, p.nblk, w.a, w.b, dgamma, dbeta, accumulate, w.u, w.v, s);
  launch_bwd_apply(p, M, C, dy, y, relu_mask, x, gamma, save_mean, save_invstd, scale, shift, relu_mode, w.u, w.v, dx, dresidual, s);
}
}  // namespace

extern "C" int ssv_bn_train_bwd(int64_t M, int32_t C, const float* dy, const float* y, const uint8_t* relu_mask, const float* x,
                                const float* gamma, const float* save_mean, const float* save_invstd, int relu,
                                float* dx, float* dresidual, float* dgamma, float* dbeta, int accumulate,
                                void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_train_bwd")) return rc;
  SSV_REQUIRE(dy && x && gamma && save_mean && save_invstd && dx && ws, "ssv_bn_train_bwd: null pointer");
  SSV_REQUIRE(!relu || y || relu_mask, "ssv_bn_train_bwd: the ReLU mask needs y or relu_mask");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_train_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_BWD, s);
  launch_bwd(M, C, dy, y, relu_mask, x, gamma, save_mean, save_invstd, nullptr, nullptr, relu ? 1 : 0, dx, dresidual, dgamma, dbeta, accumulate, ws, s);
  SSV_CHECK_LAUNCH("ssv_bn_train_bwd");
  return SSV_OK;
}

// BatchNorm + ReLU backward of the fused path: neither y nor a mask exists; the ReLU gate is x * scale + shift > 0
extern "C" int ssv_bn_relu_bwd_affine(int64_t M, int32_t C, const float* dy, const float* x, const float* gamma,
                                      const float* save_mean, const float* save_invstd, const float* scale, const float* shift,
                                      float* dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_relu_bwd_affine")) return rc;
  SSV_REQUIRE(dy && x && gamma && save_mean && save_invstd && scale && shift && dx && ws, "ssv_bn_relu_bwd_affine: null pointer");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_relu_bwd_affine: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_BWD, s);
  launch_bwd(M, C, dy, nullptr, nullptr, x, gamma, save_mean, save_invstd, scale, shift, 2, dx, nullptr, dgamma, dbeta, accumulate, ws, s);
  SSV_CHECK_LAUNCH("ssv_bn_relu_bwd_affine");
  return SSV_OK;
}

extern "C" int ssv_bn_bwd_from_partials(int64_t M, int32_t C, const float* g, const float* x, const float* gamma,
                                        const float* save_mean, const float* save_invstd, const float* psum_g, const float* psum_gx, int64_t groups,
                                        float* dx, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_bwd_from_partials")) return rc;
  SSV_REQUIRE(g && x && gamma && save_mean && save_invstd && psum_g && psum_gx && groups > 0 && groups < (1ll << 31) && dx && ws, "ssv_bn_bwd_from_partials: bad arguments");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_bwd_from_partials: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_BWD, s);
  const BnPlan p = bn_plan(M, C);
  const BnWs w = ws_vectors_first(ws, C);                     // k1 | k2 | coarse partials
  int nblk = (int)groups;
  if (int rc = coarsen_sums(C, psum_g, psum_gx, nblk, w.a, bn_coarse_floats(p, C), s)) return rc;
  launch_bwd_finalize(M, C, nblk, psum_g, psum_gx, dgamma, dbeta, accumulate, w.u, w.v, s);
  launch_bwd_apply(p, M, C, g, nullptr, nullptr, x, gamma, save_mean, save_invstd, nullptr, nullptr, 0, w.u, w.v, dx, nullptr, s);
  SSV_CHECK_LAUNCH("ssv_bn_bwd_from_partials");
  return SSV_OK;
}

// The same merge without the apply pass: the coefficients of dx = A * g + B * (x - mean) + D per channel, for consumers that form dx while
// they stage it (ssv_conv2d_fwd_dyin, ssv_conv2d_wgrad_dyin).  coef: [4][C] floats = A | mean | B | D.
extern "C" int ssv_bn_bwd_coef(int64_t M, int32_t C, const float* gamma, const float* save_mean, const float* save_invstd,
                               const float* psum_g, const float* psum_gx, int64_t groups, float* coef, float* dgamma, float* dbeta, int accumulate,
                               void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_bn_bwd_coef")) return rc;
  SSV_REQUIRE(gamma && save_mean && save_invstd && psum_g && psum_gx && groups > 0 && groups < (1ll << 31) && coef && ws, "ssv_bn_bwd_coef: bad arguments");
  SSV_REQUIRE((((uintptr_t)coef | (uintptr_t)psum_g | (uintptr_t)psum_gx) & 15) == 0, "ssv_bn_bwd_coef: pointers must be 16-byte aligned");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_bwd_coef: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_BWD, s);
  int nblk = (int)groups;
  if (int rc = coarsen_sums(C, psum_g, psum_gx, nblk, ws_vectors_first(ws, C).a, bn_coarse_floats(bn_plan(M, C), C), s)) return rc;   // as in ssv_bn_bwd_from_partials
  launch_bwd_finalize(M, C, nblk, psum_g, psum_gx, dgamma, dbeta, accumulate, nullptr, nullptr, s, gamma, save_mean, save_invstd, coef);
  SSV_CHECK_LAUNCH("ssv_bn_bwd_coef");
  return SSV_OK;
}

// ---- the image stem: BatchNorm + ReLU + MaxPool2d(3, 2, 1) as one pass each way (networks/resnet.py:147-148) ----------------
// forward : pooled = max over the window of relu(y * scale + shift); y is read once, the 112^2 activation is never written
// backward: g[pixel] = relu'(a) * sum of dpool over the (at most 2 x 2) windows whose argmax is this pixel - formed on the fly
//           in the BatchNorm backward's reduction AND apply passes, instead of materialising dy of the 112^2 map twice.  Same partition (SSV_ROW_LANE, SSV_WALK4,
//           SSV_BLOCK_TAIL2), same gather (argmax_gather) and same row (bn_bwd_acc / bn_bwd_dx) as maxpool_bwd -> bn_train_bwd: the result is bit-identical.
namespace {
__global__ void __launch_bounds__(256)
bn_relu_maxpool_fwd_k(int N, int H, int W, int C, int Ho, int Wo, const float* __restrict__ y, const float* __restrict__ scale,
                      const float* __restrict__ shift, float* __restrict__ out, uint8_t* __restrict__ am, float* __restrict__ xmax) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)N * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const PoolIdx p = pool_decode(i, C4, Wo, Ho);
    const f32x4 sc = ld4(scale + 4 * p.c4), sh = ld4(shift + 4 * p.c4);
    const PoolMax m = window_scan<true>(p, H, W, C, y, [&](f32x4 raw) {          // the ReLU of bn_apply_k
      f32x4 v = fma4(raw, sc, sh);
      v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
      return v;
    });
    st4(out + (size_t)i * 4, m.best);
    reinterpret_cast<uchar4*>(am)[i] = m.slot;
    if (xmax) st4(xmax + (size_t)i * 4, m.raw);              // the raw conv output at the arg-max pixel: the backward's pooled reduction reads it
  }
}

// gradient w.r.t. the BatchNorm output of pixel (n, hi, wi), ReLU included
__device__ __forceinline__ f32x4 pool_gate_grad(int n, int hi, int wi, int Ho, int Wo, int C4, int c4, const float* __restrict__ dpool,
                                                const uint8_t* __restrict__ am, f32x4 a) {
  return masked<true>(argmax_gather(n, hi, wi, Ho, Wo, C4, c4, dpool, am), a);
}

template <bool APPLY>
__global__ void __launch_bounds__(256)
bn_pool_bwd_k(int64_t M, int C, int CT, int RT, int rpb, int H, int W, int Ho, int Wo, const float* __restrict__ dpool, const uint8_t* __restrict__ am,
              const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ invstd,
              const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ k1, const float* __restrict__ k2,
              float* __restrict__ psg, float* __restrict__ psgx, float* __restrict__ dx) {
  __shared__ f32x4 sm1[APPLY ? 1 : 256], sm2[APPLY ? 1 : 256];
  SSV_ROW_LANE(M, C, CT, RT, rpb);
  f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
  if (active) {
    const f32x4 mu = ld4(mean + 4 * c4), is = ld4(invstd + 4 * c4), sc = ld4(scale + 4 * c4), sh = ld4(shift + 4 * c4);
    f32x4 gi = {0, 0, 0, 0}, a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
    if constexpr (APPLY) { gi = ld4(gamma + 4 * c4) * is; a1 = ld4(k1 + 4 * c4); a2 = ld4(k2 + 4 * c4); }
    // (n, hi, wi) of this thread's current row, advanced by RT pixels per visit without divisions (RT <= W is checked by the host)
    const int64_t r = r0 + rt;
    int wi = (int)(r % W);
    int hi = (int)((r / W) % H), n = (int)(r / ((int64_t)W * H));
    auto body = [&](int64_t rr) {
      const size_t o = (size_t)rr * C + 4 * c4;
      const f32x4 xv = ld4(x + o);
      const f32x4 g = pool_gate_grad(n, hi, wi, Ho, Wo, C / 4, c4, dpool, am, fma4(xv, sc, sh));
      if constexpr (APPLY) bn_bwd_dx(dx + o, g, xv, mu, is, gi, a1, a2);
      else bn_bwd_acc(g, xv, mu, is, s1, s2);
      wi += RT;
      if (wi >= W) { wi -= W; if (++hi == H) { hi = 0; ++n; } }
    };
    SSV_WALK4(r, r1, RT, body);
  }
  if constexpr (!APPLY) {
    SSV_BLOCK_TAIL2(CT, RT, sm1, sm2, s1, s2, st_partial(psg, c4, C, s1); st_partial(psgx, c4, C, s2););
  }
}
}  // namespace

extern "C" int ssv_bn_relu_maxpool_fwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* y, const float* scale, const float* shift,
                                       float* out, uint8_t* argmax, float* xmax, void* stream) {
  SSV_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "ssv_bn_relu_maxpool_fwd: bad shape (C %% 4 == 0 required)");
  SSV_REQUIRE(y && scale && shift && out && argmax, "ssv_bn_relu_maxpool_fwd: null pointer");
  const int Ho = pooled_extent(H), Wo = pooled_extent(W);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_FWD, s);
  const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(bn_relu_maxpool_fwd_k, dim3((unsigned)blocks), dim3(256), 0, s, N, H, W, C, Ho, Wo, y, scale, shift, out, argmax, xmax);
  SSV_CHECK_LAUNCH("ssv_bn_relu_maxpool_fwd");
  return SSV_OK;
}

extern "C" int ssv_bn_relu_maxpool_bwd(int32_t N, int32_t H, int32_t W, int32_t C, const float* dpool, const uint8_t* argmax, const float* y, const float* xmax,
                                       const float* gamma, const float* save_mean, const float* save_invstd, const float* scale, const float* shift,
                                       float* dy, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  const int64_t M = (int64_t)N * H * W;
  if (int rc = check_mc(M, C, "ssv_bn_relu_maxpool_bwd")) return rc;
  SSV_REQUIRE(N > 0 && H > 0 && W > 0, "ssv_bn_relu_maxpool_bwd: bad shape");
  const BnPlan p = bn_plan(M, C);
  SSV_REQUIRE(p.RT <= W, "ssv_bn_relu_maxpool_bwd: the feature map is narrower than the row stride of the kernel (W=%d)", W);
  SSV_REQUIRE(dpool && argmax && y && gamma && save_mean && save_invstd && scale && shift && dy && ws, "ssv_bn_relu_maxpool_bwd: null pointer");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_bn_relu_maxpool_bwd: workspace too small");
  const int Ho = pooled_extent(H), Wo = pooled_extent(W);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_BN_BWD, s);
  const BnWs w = ws_partials_first(ws, p, C);                 // psg | psgx | k1 | k2
  const dim3 grid(p.nblk, p.GY);
  const int64_t Mp = (int64_t)N * Ho * Wo;
  const BnPlan pp = bn_plan(Mp, C);
  int nred = p.nblk;
  if (xmax && pp.nblk > p.nblk) xmax = nullptr;               // the pooled plan's partials must fit the workspace laid out above (they do unless rounding gives the pooled plan more blocks: 449 x 11 x 11 x 256 has 1011 against 1007)
  if (xmax) {
    // Reduction at the POOLED resolution (round 4): sum g and sum g * xhat over the 112^2 map are sums over the pooled positions - a pixel's g is the sum of
    // the dpool of the windows whose arg-max it is, gated by the ReLU bit of that pixel, and the forward kept the raw conv output of every window's arg-max
    // pixel (xmax) - so the pass reads dpool and xmax (2 x 1/4 of the map) instead of walking the full-resolution conv output: the generic reduction
    // kernel with the recomputed gate, on [N*Ho*Wo][C].  Same terms as the full-resolution walk, grouped per window instead of per pixel (rounding-level).
    nred = pp.nblk;
    hipLaunchKernelGGL((bn_bwd_reduce_k<2>), dim3(pp.nblk, pp.GY), dim3(256), 0, s, Mp, C, pp.CT, pp.RT, pp.rpb, dpool, (const float*)nullptr,
                       (const uint8_t*)nullptr, xmax, save_mean, save_invstd, scale, shift, w.a, w.b);
  } else {
    hipLaunchKernelGGL((bn_pool_bwd_k<false>), grid, dim3(256), 0, s, M, C, p.CT, p.RT, p.rpb, H, W, Ho, Wo, dpool, argmax, y, gamma, save_mean, save_invstd,
                       scale, shift, (const float*)nullptr, (const float*)nullptr, w.a, w.b, (float*)nullptr);
  }
  launch_bwd_finalize(M, C, nred, w.a, w.b, dgamma, dbeta, accumulate, w.u, w.v, s);
  hipLaunchKernelGGL((bn_pool_bwd_k<true>), grid, dim3(256), 0, s, M, C, p.CT, p.RT, p.rpb, H, W, Ho, Wo, dpool, argmax, y, gamma, save_mean, save_invstd,
                     scale, shift, (const float*)w.u, (const float*)w.v, (float*)nullptr, (float*)nullptr, dy);
  SSV_CHECK_LAUNCH("ssv_bn_relu_maxpool_bwd");
  return SSV_OK;
}

extern "C" int ssv_colsum(int64_t M, int32_t C, const float* x, float* out, int accumulate,
                          void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_mc(M, C, "ssv_colsum")) return rc;
  SSV_REQUIRE(x && out && ws, "ssv_colsum: null pointer");
  if (ws_bytes < ssv_bn_workspace_bytes(M, C)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_colsum: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  const BnPlan p = bn_plan(M, C);
  float* part = (float*)ws;
  hipLaunchKernelGGL(colsum_partial_k, dim3(p.nblk, p.GY), dim3(256), 0, s, M, C, p.CT, p.RT, p.rpb, x, part);
  hipLaunchKernelGGL(colsum_finalize_k, dim3(cdiv(C, FIN_C)), dim3(256), 0, s, C, p.nblk, (const float*)part, out, accumulate);
  SSV_CHECK_LAUNCH("ssv_colsum");
  return SSV_OK;
}
