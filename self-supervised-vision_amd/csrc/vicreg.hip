// VICReg (Bardes, Ponce, LeCun 2022): the element-wise work around the loss's GEMMs (include/ssv_hip.h states the formulas and the sequence of launches).
// For x, y [B][D]:  loss = sim_coeff mean (x - y)^2 + std_coeff (mean_j relu(1 - s_x[j]) + mean_j relu(1 - s_y[j])) / 2 + cov_coeff (|offdiag C_x|^2 + |offdiag C_y|^2) / D
// with xc = x - mean_b(x), s_x = sqrt(var_unbiased + eps), C_x = xc^T xc / (B - 1), and
//     dx = 2 sim_coeff (x - y) / (B D)  -  std_coeff / (2 D (B - 1)) xc[:, j] / s_x[j] [s_x[j] < 1]  +  4 cov_coeff / (D (B - 1)) xc offdiag(C_x).
// THE CENTRING HAS NO BACKWARD OF ITS OWN.  dL/dx = (I - 11^T / B) dL/dxc, and both terms of dL/dxc have zero column mean: the hinge term is a column of xc times a
// scalar, the covariance term is xc times a matrix, and the columns of xc sum to zero.  So the projection is the identity on them and dL/dx = dL/dxc
// (tests/test_vicreg_cpu.py holds the column means to rounding).  The sim term does not pass through the centring at all.
//
//   vicreg_prep_k   one workgroup per strip of 32 columns - 128-byte row segments, 8 lanes of 16 bytes, 32 rows per trip of the 256 threads - for BOTH views,
//                   three walks over the rows:  (1) column sums of x and y -> means;  (2) x and y again: xc, yc and the sim term g (x - y) / -g (x - y) of e
//                   written, centred squares and (x - y)^2 summed -> s, the hinge and its coefficient per column;  (3) where a column's hinge is active, the
//                   thread re-reads the xc and e it wrote itself and adds coefficient * xc to e.  x and y come from HBM twice each; a strip whose hinges are all
//                   inactive ends after (2) and its e is the sim term bit for bit.  The variance is the sum of centred squares, never E[x^2] - mean^2.
//                   Sums per thread in double, the 32 row groups added in order through LDS; the strip's two partials go to ws[strip].
//   vicreg_cgrad_k  grid-stride over craw [2][D][D] in float4s: the off-diagonal squares of craw / (B - 1) summed in double into ws[block]; in place
//                   G = gscale * craw, 0 on the diagonal.
//   the two fold kernels add the partials of ws in index order (one workgroup, a fixed tree) and write parts[2] / loss[4].
// No floating-point atomics anywhere: equal inputs give equal bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int STRIP = 32;          // columns per workgroup: 128 bytes of every row
constexpr int ROWS = 32;           // rows per trip: 256 threads = 32 rows x 8 lanes x 4 columns
constexpr int CGRAD_MAX_BLOCKS = 1024;

__global__ void __launch_bounds__(256)
vicreg_prep_k(int B, int D, const float* __restrict__ x, const float* __restrict__ y, float g_sim, float c_std, float eps,
              float* xc, float* __restrict__ s, float* e, double* __restrict__ part) {
  __shared__ double red[3][ROWS][STRIP];
  __shared__ double colp[3][STRIP];
  __shared__ float mean_s[2][STRIP];
  __shared__ float coef_s[2][STRIP];
  const int q = threadIdx.x & 7, rg = threadIdx.x >> 3;
  const int64_t col0 = (int64_t)blockIdx.x * STRIP + 4 * q;            // col0 + 3 < D: D % 32 == 0 and gridDim.x == D / 32
  const int64_t BD = (int64_t)B * D;

  // (1) column sums
  double sx[4] = {0.0, 0.0, 0.0, 0.0}, sy[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int r = rg; r < B; r += ROWS) {
    const int64_t off = (int64_t)r * D + col0;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + off);
#pragma unroll
    for (int k = 0; k < 4; ++k) { sx[k] += (double)xv[k]; sy[k] += (double)yv[k]; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { red[0][rg][4 * q + k] = sx[k]; red[1][rg][4 * q + k] = sy[k]; }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int v = threadIdx.x >> 5, c = threadIdx.x & 31;
    double t = 0.0;
    for (int i = 0; i < ROWS; ++i) t += red[v][i][c];
    mean_s[v][c] = (float)(t / (double)B);
  }
  __syncthreads();

  // (2) centred values, the sim term of e, centred squares and squared differences
  float mx[4], my[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { mx[k] = mean_s[0][4 * q + k]; my[k] = mean_s[1][4 * q + k]; }
  double vx[4] = {0.0, 0.0, 0.0, 0.0}, vy[4] = {0.0, 0.0, 0.0, 0.0}, ds[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
  for (int r = rg; r < B; r += ROWS) {
    const int64_t off = (int64_t)r * D + col0;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + off);
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + off);
    f32x4 cx, cy, ex, ey;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cx[k] = xv[k] - mx[k];
      cy[k] = yv[k] - my[k];
      const float d = xv[k] - yv[k];
      ex[k] = g_sim * d;
      ey[k] = -ex[k];
      vx[k] = __builtin_fma((double)cx[k], (double)cx[k], vx[k]);
      vy[k] = __builtin_fma((double)cy[k], (double)cy[k], vy[k]);
      ds[k] = __builtin_fma((double)d, (double)d, ds[k]);
    }
    *reinterpret_cast<f32x4*>(xc + off) = cx;
    *reinterpret_cast<f32x4*>(xc + BD + off) = cy;
    *reinterpret_cast<f32x4*>(e + off) = ex;
    *reinterpret_cast<f32x4*>(e + BD + off) = ey;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { red[0][rg][4 * q + k] = vx[k]; red[1][rg][4 * q + k] = vy[k]; red[2][rg][4 * q + k] = ds[k]; }
  __syncthreads();
  if (threadIdx.x < 96) {
    const int v = threadIdx.x >> 5, c = threadIdx.x & 31;
    double t = 0.0;
    for (int i = 0; i < ROWS; ++i) t += red[v][i][c];
    if (v < 2) {
      const float sd = (float)sqrt(t / (double)(B - 1) + (double)eps);
      const bool active = sd < 1.f;                                     // relu(1 - s) has slope 0 at s == 1 and beyond; a NaN s is inactive
      s[(int64_t)v * D + (int64_t)blockIdx.x * STRIP + c] = sd;
      colp[v][c] = active ? (double)(1.f - sd) : 0.0;
      coef_s[v][c] = (active && c_std != 0.f) ? c_std / sd : 0.f;
    } else {
      colp[2][c] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sim = 0.0, hinge = 0.0;
    for (int c = 0; c < STRIP; ++c) sim += colp[2][c];
    for (int c = 0; c < STRIP; ++c) hinge += colp[0][c];
    for (int c = 0; c < STRIP; ++c) hinge += colp[1][c];
    part[2 * (int64_t)blockIdx.x] = sim;
    part[2 * (int64_t)blockIdx.x + 1] = hinge;
  }

  // (3) the hinge term, on the elements this thread wrote itself
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    float cf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cf[k] = coef_s[v][4 * q + k];
    if (cf[0] == 0.f && cf[1] == 0.f && cf[2] == 0.f && cf[3] == 0.f) continue;
    for (int r = rg; r < B; r += ROWS) {
      const int64_t off = (int64_t)v * BD + (int64_t)r * D + col0;
      const f32x4 cv = *reinterpret_cast<const f32x4*>(xc + off);
      f32x4 ev = *reinterpret_cast<const f32x4*>(e + off);
#pragma unroll
      for (int k = 0; k < 4; ++k) if (cf[k] != 0.f) ev[k] = __builtin_fmaf(cf[k], cv[k], ev[k]);
      *reinterpret_cast<f32x4*>(e + off) = ev;
    }
  }
}

__global__ void __launch_bounds__(64)
vicreg_prep_fold_k(int strips, const double* __restrict__ part, double sim_scale, double std_scale, float* __restrict__ parts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sim = 0.0, hinge = 0.0;
  for (int i = 0; i < strips; ++i) { sim += part[2 * i]; hinge += part[2 * i + 1]; }
  parts[0] = (float)(sim_scale * sim);
  parts[1] = (float)(std_scale * hinge);
}

__global__ void __launch_bounds__(256)
vicreg_cgrad_k(uint32_t D, uint32_t n4, float* __restrict__ craw, double inv_bm1, float gscale, double* __restrict__ part) {
  __shared__ double sm[256];
  const uint32_t dd = D * D;                                            // <= 2^26; 4 * n4 = 2 * dd <= 2^27
  double acc = 0.0;
  for (uint32_t i4 = blockIdx.x * 256u + threadIdx.x; i4 < n4; i4 += gridDim.x * 256u) {
    const uint32_t i = 4u * i4, idx = i >= dd ? i - dd : i;
    const uint32_t r = idx / D, c = idx - r * D;                        // D % 4 == 0: the four elements share the row
    const f32x4 v = reinterpret_cast<const f32x4*>(craw)[i4];
    f32x4 g;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool diag = c + k == r;
      const double cv = (double)v[k] * inv_bm1;
      if (!diag) acc = __builtin_fma(cv, cv, acc);
      g[k] = diag ? 0.f : gscale * v[k];
    }
    reinterpret_cast<f32x4*>(craw)[i4] = g;
  }
  sm[threadIdx.x] = acc;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

__global__ void __launch_bounds__(256)
vicreg_cgrad_fold_k(int nb, const double* __restrict__ part, double cov_scale, const float* __restrict__ parts, float* __restrict__ loss) {
  __shared__ double sm[256];
  double t = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) t += part[i];
  sm[threadIdx.x] = t;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) {
    const float sim = parts[0], sd = parts[1], cov = (float)(cov_scale * sm[0]);
    loss[0] = (sim + sd) + cov;
    loss[1] = sim;
    loss[2] = sd;
    loss[3] = cov;
  }
}

bool shape_ok(int32_t B, int32_t D) {
  return B >= 2 && D >= 32 && D % 32 == 0 && D <= SSV_KNN_MAX_D && (int64_t)B * D <= ((int64_t)1 << 30);
}
bool coeff_ok(float c) { return __builtin_isfinite(c) && c >= 0.f; }
int cgrad_blocks(int32_t D) {
  const int64_t n4 = (int64_t)D * D / 2;
  const int64_t b = cdiv64(n4, 256 * 4);
  return (int)(b > CGRAD_MAX_BLOCKS ? CGRAD_MAX_BLOCKS : b);
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t ssv_vicreg_workspace_bytes(int32_t B, int32_t D) {
  if (!shape_ok(B, D)) return 0;
  const size_t prep = (size_t)(D / STRIP) * 2, cg = (size_t)cgrad_blocks(D);
  return up256((prep > cg ? prep : cg) * sizeof(double));
}

extern "C" int ssv_vicreg_prep(int32_t B, int32_t D, const float* x, const float* y, float sim_coeff, float std_coeff, float cov_coeff, float eps,
                               float* xc, float* s_out, float* e, float* parts, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(B, D), "ssv_vicreg_prep: need B >= 2, D a multiple of 32 in [32, %d] and B * D <= 2^30 (got B=%d D=%d)", SSV_KNN_MAX_D, B, D);
  SSV_REQUIRE(coeff_ok(sim_coeff) && coeff_ok(std_coeff) && coeff_ok(cov_coeff), "ssv_vicreg_prep: the coefficients must be finite and >= 0 (got %g %g %g)",
              (double)sim_coeff, (double)std_coeff, (double)cov_coeff);
  SSV_REQUIRE(coeff_ok(eps), "ssv_vicreg_prep: eps must be finite and >= 0 (got %g)", (double)eps);
  SSV_REQUIRE(x && y && xc && s_out && e && parts && ws, "ssv_vicreg_prep: null pointer");
  SSV_REQUIRE(aligned16(x) && aligned16(y) && aligned16(xc) && aligned16(e) && aligned16(ws), "ssv_vicreg_prep: x, y, xc, e and ws must be 16-byte aligned");
  const size_t need = ssv_vicreg_workspace_bytes(B, D);
  SSV_REQUIRE(ws_bytes >= need, "ssv_vicreg_prep: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, st);
  const int strips = D / STRIP;
  const double bd = (double)B * (double)D;
  const float g_sim = (float)(2.0 * (double)sim_coeff / bd);
  const float c_std = (float)(-(double)std_coeff / (2.0 * (double)D * (double)(B - 1)));
  hipLaunchKernelGGL(vicreg_prep_k, dim3(strips), dim3(256), 0, st, (int)B, (int)D, x, y, g_sim, c_std, eps, xc, s_out, e, (double*)ws);
  SSV_CHECK_LAUNCH("vicreg_prep_k");
  hipLaunchKernelGGL(vicreg_prep_fold_k, dim3(1), dim3(64), 0, st, strips, (const double*)ws, (double)sim_coeff / bd, (double)std_coeff / (2.0 * (double)D), parts);
  SSV_CHECK_LAUNCH("vicreg_prep_fold_k");
  return SSV_OK;
}

extern "C" int ssv_vicreg_cgrad(int32_t B, int32_t D, float* craw, float cov_coeff, const float* parts, float* loss, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(shape_ok(B, D), "ssv_vicreg_cgrad: need B >= 2, D a multiple of 32 in [32, %d] and B * D <= 2^30 (got B=%d D=%d)", SSV_KNN_MAX_D, B, D);
  SSV_REQUIRE(coeff_ok(cov_coeff), "ssv_vicreg_cgrad: cov_coeff must be finite and >= 0 (got %g)", (double)cov_coeff);
  SSV_REQUIRE(craw && parts && loss && ws, "ssv_vicreg_cgrad: null pointer");
  SSV_REQUIRE(aligned16(craw) && aligned16(ws), "ssv_vicreg_cgrad: craw and ws must be 16-byte aligned");
  const size_t need = ssv_vicreg_workspace_bytes(B, D);
  SSV_REQUIRE(ws_bytes >= need, "ssv_vicreg_cgrad: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, st);
  const int nb = cgrad_blocks(D);
  const double bm1 = (double)(B - 1);
  const float gscale = (float)(4.0 * (double)cov_coeff / ((double)D * bm1 * bm1));
  hipLaunchKernelGGL(vicreg_cgrad_k, dim3(nb), dim3(256), 0, st, (uint32_t)D, (uint32_t)((int64_t)D * D / 2), craw, 1.0 / bm1, gscale, (double*)ws);
  SSV_CHECK_LAUNCH("vicreg_cgrad_k");
  hipLaunchKernelGGL(vicreg_cgrad_fold_k, dim3(1), dim3(256), 0, st, nb, (const double*)ws, (double)cov_coeff / (double)D, parts, loss);
  SSV_CHECK_LAUNCH("vicreg_cgrad_fold_k");
  return SSV_OK;
}
