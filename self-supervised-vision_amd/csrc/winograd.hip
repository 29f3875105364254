// Winograd F(2x2, 3x3) for the stride-1 3x3 convolutions of the deep stages (networks/resnet.py:7-10, 56-58: conv3x3, padding 1).
//
// These layers are MFMA-bound at exact fp32 (102 - 128 TFLOP/s of a 157 TFLOP/s pipe): the only way past that roof without changing the
// arithmetic type is fewer multiplies.  F(2x2, 3x3) computes a 2x2 output tile from a 4x4 input tile with 16 multiplies per
// (input channel, output channel) instead of 36:
//
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A        V = B^T d B   U = G g G^T   M[xi][nu] = sum_c V[xi][nu][c] U[xi][nu][c]
//
// i.e. 16 independent GEMMs  M_p [T x K] = V_p [T x C] . U_p^T [C x K]  (p = 4 xi + nu, T = N * ceil(H/2) * ceil(W/2) tiles), which run as ONE
// batched launch of the implicit-GEMM kernel (conv_mfma.hip, blockIdx.y = p).  The transforms are streaming kernels (this file):
//
//   wino_filter_k   g [K][3][3][C] (OHWI)      -> U [16][K][C]                      once per weight and step
//   wino_input_k    x [N][H][W][C] (+ fused BatchNorm + ReLU of the producer)  -> V [16][T][C]
//   wino_output_k   M [16][T][K]               -> y [N][H][W][K]  (+ BatchNorm statistics partials | + ReLU gate and its partial sums)
//   wino_dy_k       dy [N][H][W][K]            -> dM [16][T][K] = A dY A^T          weight gradient: dU_p = dM_p^T . V_p  (V kept from the forward)
//   wino_dfilter_k  dU [16][K][C]              -> dg (+)= G^T dU G
//
// All arithmetic is fp32; the transforms use only additions and multiplications by 1/2 (exact), so the result differs from the direct
// convolution by summation order and by the rounding of the transformed operands (measured against fp64 next to the direct kernel:
// tools/probe_winograd.py, profiles/r03_probe_winograd.txt).
#include "winograd_tile.h"

namespace {

// ---- filter: U[p][k][c] = (G g G^T)[xi][nu],  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]] -------------------------------------
__global__ void __launch_bounds__(256)
wino_filter_k(int K, int C, const float* __restrict__ g, float* __restrict__ U) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;          // (k, c)
  if (idx >= (int64_t)K * C) return;
  const int k = (int)(idx / C), c = (int)(idx - (int64_t)k * C);
  float w[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) w[r][s] = g[((size_t)k * 9 + r * 3 + s) * C + c];
  float t[4][3];                       // G g : per filter column s
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    float col[3], u[4];
#pragma unroll
    for (int r = 0; r < 3; ++r) col[r] = w[r][s];
    g4(col, u);
#pragma unroll
    for (int a = 0; a < 4; ++a) t[a][s] = u[a];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float u[4];
    g4(t[a], u);
    const size_t o = (size_t)(a * 4) * K * C + (size_t)k * C + c;
    U[o] = u[0]; U[o + (size_t)K * C] = u[1]; U[o + 2 * (size_t)K * C] = u[2]; U[o + 3 * (size_t)K * C] = u[3];
  }
}

// dg[k][r][s][c] (+)= (G^T dU G)[r][s]
__global__ void __launch_bounds__(256)
wino_dfilter_k(int K, int C, const float* __restrict__ dU, float* __restrict__ dg, int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)K * C) return;
  const int k = (int)(idx / C), c = (int)(idx - (int64_t)k * C);
  float u[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) u[a][b] = dU[(size_t)(a * 4 + b) * K * C + (size_t)k * C + c];
  float t[3][4];                       // G^T u: rows
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    float col[4], r[3];
#pragma unroll
    for (int a = 0; a < 4; ++a) col[a] = u[a][b];
    gt4(col, r);
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q][b] = r[q];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float d[3];
    gt4(t[r], d);
    float* o = dg + ((size_t)k * 9 + r * 3) * C + c;
    if (accumulate) { o[0] += d[0]; o[C] += d[1]; o[2 * (size_t)C] += d[2]; }
    else { o[0] = d[0]; o[C] = d[1]; o[2 * (size_t)C] = d[2]; }
  }
}

// ---- input: V[p][t][c] = (B^T d B)[xi][nu] over the 4x4 patch of tile t (rows 2i-1 .. 2i+2, zero outside the image) -----------
// One thread = one tile x 4 channels; the lanes of a wave run along the channels, so every load / store is a whole contiguous row segment.
// XF: x is the producer's raw conv output and the operand is relu(x * scale[c] + shift[c]) - same fmaf / fmaxf as bn_apply_k; padding stays 0.
template <bool XF>
__global__ void __launch_bounds__(256)
wino_input_k(int N, int H, int W, int C, int th, int tw, const float* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
             float* __restrict__ V, int64_t T) {
  const int C4 = C >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= T * C4) return;
  const int64_t t = idx / C4;
  const int c = (int)(idx - t * C4) * 4;
  const TileAt at = tile_at(t, th, tw);
  const int n = at.n, i = at.i, j = at.j;
  f32x4 scv = {1.f, 1.f, 1.f, 1.f}, shv = {0.f, 0.f, 0.f, 0.f};
  if constexpr (XF) { scv = ldv<4>(sc + c); shv = ldv<4>(sh + c); }
  f32x4 d[4][4];
  SSV_WINO_LOAD_PATCH(4, 4, 2, d, x, n, i, j, H, W, C, c,
    if constexpr (XF) { _Pragma("unroll") for (int e = 0; e < 4; ++e) v[e] = fmaxf(__builtin_fmaf(v[e], scv[e], shv[e]), 0.f); });
  SSV_WINO22_TRANSFORM_STORE(4, 4, d, 0, 0, V + (size_t)t * C + c, (size_t)T * C, Bt4);
}

// ---- weight gradient operand: dM[p][t][k] = (A dY A^T)[xi][nu],  A^T = [[1,1,1,0],[0,1,-1,-1]] ----------------------------------
__global__ void __launch_bounds__(256)
wino_dy_k(int N, int H, int W, int K, int th, int tw, const float* __restrict__ dy, float* __restrict__ dM, int64_t T) {
  const int K4 = K >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= T * K4) return;
  const int64_t t = idx / K4;
  const int k = (int)(idx - t * K4) * 4;
  const TileAt at = tile_at(t, th, tw);
  const int n = at.n, i = at.i, j = at.j;
  f32x4 y[2][2];
  load_tile<4, 2>(y, dy, n, i, j, H, W, K, k);
  SSV_WINO22_TRANSFORM_STORE(4, 2, y, 0, 0, dM + (size_t)t * K + k, (size_t)T * K, A4);
}

// ---- output: y = A^T M A per tile; one workgroup = one GROUP of 16 consecutive tiles x a run of <= 1024 channels ----------------
// MODE 0 plain | 1 statistics: the group's output rows reduced per channel to (mean, centred sum of squares), one partial per group - the layout
// ssv_bn_stats_finalize takes with rows_per_group = ssv_wino_stats_rows_per_group (every group must hold the same number of rows) | 2 gate: y is the gradient w.r.t. a
// BatchNorm + ReLU output whose input is gx: store g = (gx * gscale + gshift > 0) ? y : 0 and the group's sums of g and g * xhat | 3 the same
// with the ReLU bit taken from the forward's byte mask (one byte per four channels, ssv_bn_apply).
constexpr int WG_TILES = 16;
template <int MODE>
__global__ void __launch_bounds__(256)
wino_output_k(int N, int H, int W, int K, int th, int tw, const float* __restrict__ M, float* __restrict__ y, int64_t T,
              float* __restrict__ p0, float* __restrict__ p1, const float* __restrict__ gx, const float* __restrict__ gscale,
              const float* __restrict__ gshift, const float* __restrict__ gmean, const float* __restrict__ ginvstd, const uint8_t* __restrict__ gmask) {
  __shared__ float red[3][256 * 4];
  const int K4 = K >> 2;
  const int L = K4 < 256 ? K4 : 256;          // lanes along the channels
  const int TPP = 256 / L;                    // tiles per pass
  const int tid = threadIdx.x;
  const int lc = tid % L, ts = tid / L;
  const int k = (blockIdx.y * 256 + lc) * 4;
  const bool kok = k < K && ts < TPP;
  const int64_t g0 = (int64_t)blockIdx.x * WG_TILES;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = {0.f, 0.f, 0.f, 0.f}, gs = {0.f, 0.f, 0.f, 0.f}, gh = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.f;
  if constexpr (MODE >= 2) { if (kok) { mu = ldv<4>(gmean + k); is = ldv<4>(ginvstd + k); } }
  if constexpr (MODE == 2) { if (kok) { gs = ldv<4>(gscale + k); gh = ldv<4>(gshift + k); } }
  const size_t ps = (size_t)T * K;
  for (int p = 0; p < WG_TILES; p += TPP) {
    const int64_t t = g0 + p + ts;
    // K < 64: TPP > WG_TILES, and the lanes past the group's 16 tiles idle - the tiles behind them belong to the following groups, whose partials they
    // must not enter (tests/test_gpu_wino_forms.py, lanes.lt16, holds this group by group at K = 32)
    if (!kok || p + ts >= WG_TILES || t >= T) continue;
    const TileAt at = tile_at(t, th, tw);
    const int n = at.n, i = at.i, j = at.j;
    const float* mp = M + (size_t)t * K + k;
    f32x4 m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) m[a][b] = ldv<4>(mp + (size_t)(a * 4 + b) * ps);
    f32x4 s[2][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f32x4 col[4], o[2];
#pragma unroll
      for (int a = 0; a < 4; ++a) col[a] = m[a][b];
      at4(col, o);
      s[0][b] = o[0]; s[1][b] = o[1];
    }
    f32x4 tv[MODE == 1 ? 4 : 1], tsum = {0.f, 0.f, 0.f, 0.f};          // statistics: this tile's pixels, their sum and count
    float tcnt = 0.f;
    unsigned tok = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      f32x4 o[2];
      at4(s[a], o);
      const int ho = 2 * i + a;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int wo = 2 * j + b;
        if (ho >= H || wo >= W) continue;
        f32x4 v = o[b];
        const size_t off = (((size_t)n * H + ho) * W + wo) * K + k;
        if constexpr (MODE >= 2) {
          const f32x4 xv = ldv<4>(gx + off);
          if constexpr (MODE == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(xv[e], gs[e], gh[e]) > 0.f ? v[e] : 0.f;
          } else {
            const unsigned bits = gmask[off >> 2];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (bits >> e) & 1u ? v[e] : 0.f;
          }
          s1 += v;
          s2 += v * ((xv - mu) * is);
        }
        if constexpr (MODE == 1) { tv[a * 2 + b] = v; tsum += v; tcnt += 1.f; tok |= 1u << (a * 2 + b); }
        stv<4>(y + off, v);
      }
    }
    if constexpr (MODE == 1) {
      // the tile's (count, mean, M2) about its own mean, merged into the thread's running triple (s1 = mean, s2 = M2) as the LDS merge below merges the threads'.
      // (A running sum about the thread's first pixel lost a digit on every channel whose first pixel was an outlier: at K = 1024, one thread per channel over 64
      // rows, the mean sat 16x further from fp64 than a pairwise fp32 mean - tests/test_gpu_wino_forms.py, stats.g64 at lanes.one, holds the partials to 8x.)
      const f32x4 tmean = tsum / tcnt;                                   // pixel (0, 0) of an existing tile is always inside the map: tcnt >= 1
      f32x4 tm2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((tok >> q) & 1u) { const f32x4 dv = tv[q] - tmean; tm2 += dv * dv; }
      if (cnt == 0.f) { s1 = tmean; s2 = tm2; cnt = tcnt; }
      else {
        const float tot = cnt + tcnt;
        const f32x4 dlt = tmean - s1;
        s2 += tm2 + dlt * dlt * (cnt * tcnt / tot);
        s1 += dlt * (tcnt / tot);
        cnt = tot;
      }
    }
  }
  if constexpr (MODE == 0) return;
  // merge the TPP partial results per channel in fixed order (thread ts == 0 of each channel lane)
  if constexpr (MODE == 1) merge_stats<4>(red, s1, s2, cnt, L, TPP, lc, ts, kok, p0, p1, K, k);          // this thread's (count, mean, M2)
  else merge_sums<4>(red, s1, s2, L, TPP, lc, ts, kok, p0, p1, K, k);
}

}  // namespace

extern "C" int64_t ssv_wino_tiles(int32_t N, int32_t H, int32_t W) {
  return (N > 0 && H > 0 && W > 0) ? (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) : 0;
}

extern "C" int64_t ssv_wino_groups(int32_t N, int32_t H, int32_t W) { return cdiv64(ssv_wino_tiles(N, H, W), WG_TILES); }

// Output rows every statistics partial of ssv_wino_output_transform summarises (the rows_per_group to hand ssv_bn_stats_finalize), or 0 when the
// map does not partition evenly: 64 when every tile is whole (H, W even: 16 tiles x 4 rows); H * W when one image is exactly one group of 16
// tiles (7x7 and 8x7 .. maps: ceil(H/2) * ceil(W/2) == 16).
extern "C" int32_t ssv_wino_stats_rows_per_group(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  if (H % 2 == 0 && W % 2 == 0) return 4 * WG_TILES;
  if (((H + 1) / 2) * ((W + 1) / 2) == WG_TILES) return H * W;
  return 0;
}

extern "C" int ssv_wino_filter_transform(int32_t K, int32_t C, const float* w, float* U, void* stream) {
  return wino_launch_kc("ssv_wino_filter_transform", SSV_PROF_MISC, wino_filter_k, K, C, w, U, stream);
}

extern "C" int ssv_wino_filter_grad(int32_t K, int32_t C, const float* dU, float* dw, int accumulate, void* stream) {
  return wino_launch_kc("ssv_wino_filter_grad", SSV_PROF_CONV_WGRAD, wino_dfilter_k, K, C, dU, dw, stream, accumulate);
}

extern "C" int ssv_wino_input_transform(int32_t N, int32_t H, int32_t W, int32_t C, const float* x, const float* in_scale, const float* in_shift,
                                        float* V, void* stream) {
  if (int rc = wino_check_shape(N, H, W, C, "ssv_wino_input_transform")) return rc;
  SSV_REQUIRE(x && V && (in_scale == nullptr) == (in_shift == nullptr), "ssv_wino_input_transform: bad pointers");
  SSV_REQUIRE((((uintptr_t)x | (uintptr_t)V | (uintptr_t)in_scale | (uintptr_t)in_shift) & 15) == 0, "ssv_wino_input_transform: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_CONV_FWD, s);
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  const int64_t T = (int64_t)N * th * tw;
  const dim3 grid((unsigned)cdiv64(T * (C / 4), 256));
  if (in_scale) hipLaunchKernelGGL(wino_input_k<true>, grid, dim3(256), 0, s, N, H, W, C, th, tw, x, in_scale, in_shift, V, T);
  else hipLaunchKernelGGL(wino_input_k<false>, grid, dim3(256), 0, s, N, H, W, C, th, tw, x, in_scale, in_shift, V, T);
  SSV_CHECK_LAUNCH("ssv_wino_input_transform");
  return SSV_OK;
}

extern "C" int ssv_wino_dy_transform(int32_t N, int32_t H, int32_t W, int32_t K, const float* dy, float* dM, void* stream) {
  if (int rc = wino_check_shape(N, H, W, K, "ssv_wino_dy_transform")) return rc;
  SSV_REQUIRE(dy && dM && (((uintptr_t)dy | (uintptr_t)dM) & 15) == 0, "ssv_wino_dy_transform: null or unaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_CONV_WGRAD, s);
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  const int64_t T = (int64_t)N * th * tw;
  hipLaunchKernelGGL(wino_dy_k, dim3((unsigned)cdiv64(T * (K / 4), 256)), dim3(256), 0, s, N, H, W, K, th, tw, dy, dM, T);
  SSV_CHECK_LAUNCH("ssv_wino_dy_transform");
  return SSV_OK;
}

// y = A^T M A.  Optional (at most one): statistics partials (pmean, pm2: [ssv_wino_groups][K], 64 rows per group - H and W must be even) or a
// ReLU gate with its partial sums (gate->x / mean / invstd / psum_g / psum_gx: [ssv_wino_groups][K]; byte mask or scale + shift; no second target).
extern "C" int ssv_wino_output_transform(int32_t N, int32_t H, int32_t W, int32_t K, const float* M, float* y, float* pmean, float* pm2,
                                         const ssv_bn_gate* gate, void* stream) {
  if (int rc = wino_check_output(N, H, W, K, M, y, pmean, pm2, gate, 4, ssv_wino_stats_rows_per_group(N, H, W) > 0, "ssv_wino_output_transform")) return rc;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(gate ? SSV_PROF_CONV_DGRAD : SSV_PROF_CONV_FWD, s);
  const int th = (H + 1) / 2, tw = (W + 1) / 2;
  const int64_t T = (int64_t)N * th * tw;
  const dim3 grid((unsigned)cdiv64(T, WG_TILES), (unsigned)cdiv(K / 4, 256));
  SSV_WINO_MODE_LADDER(wino_output_k, grid, s, gate, pmean, pm2, N, H, W, K, th, tw, M, y, T);
  SSV_CHECK_LAUNCH("ssv_wino_output_transform");
  return SSV_OK;
}
