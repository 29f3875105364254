// What the two Winograd forms share, written once: F(2x2, 3x3) (csrc/winograd.hip: tile edge 2, patch edge 4, 16 positions, 4 channels per thread) and
// F(4x4, 3x3) (csrc/winograd44.hip: 4, 6, 36, 4 or 2 channels per thread) are the same kernels with different numbers.  Included by those two files only.
//   device  vecf / ldv / stv, the tile walk (tile_at), the zero-padded patch load (SSV_WINO_LOAD_PATCH) and the output-tile load (load_tile), the 1-D transforms
//           of both forms side by side, the two-sided transform with its position-by-position store (SSV_WINO_TRANSFORM_STORE, SSV_WINO22_TRANSFORM_STORE) and
//           the two LDS merge tails of the output transforms (merge_stats, merge_sums)
//   host    the argument checks and launch spellings of the entry points
// Three identities the sources promise hold by construction, because both sides expand the same text: V2 of wino44_input_k<.., BOTH> == wino_input_k's output
// (the patch load + SSV_WINO22_TRANSFORM_STORE over Bt4), Vd of wino44_dy_both_k == wino44_input_k<.., false, false>'s output (the patch load +
// SSV_WINO_TRANSFORM_STORE over Bt6) and its dM == wino44_dy_k's (SSV_WINO_TRANSFORM_STORE over A6); tests/test_gpu_wino_forms.py, identity (e), holds them on
// the GPU.  Every kernel is, instruction for instruction, the machine code it was when each carried its own copy of these lines (tools/isa_compare.py,
// profiles/wino_once_isa_vs_parent.json); where that needed text instead of a function, the comment at the macro says what the function form changed.
#pragma once
#include "common.h"

namespace {

// ---- vector access: VW consecutive channels of one pixel / position ------------------------------------------------------------------------------------
template <int VW> using vecf = float __attribute__((ext_vector_type(VW)));
template <int VW> __device__ __forceinline__ vecf<VW> ldv(const float* p) { return *reinterpret_cast<const vecf<VW>*>(p); }
template <int VW> __device__ __forceinline__ void stv(float* p, vecf<VW> v) { *reinterpret_cast<vecf<VW>*>(p) = v; }

// ---- tile walk: tile t of the order (n, i, j) over th x tw tiles per image -------------------------------------------------------------------------------
struct TileAt { int n, i, j; };
__device__ __forceinline__ TileAt tile_at(int64_t t, int th, int tw) {
  const int n = (int)(t / (th * tw));
  const int r = (int)(t - (int64_t)n * th * tw);
  const int i = r / tw;
  return {n, i, r - i * tw};
}

// the P x P input patch of tile (i, j): rows STEP * i - 1 .. of image n, zero outside the image.  FORM is a statement that may rewrite the loaded element v (at
// element offset off) in place - the BatchNorm + ReLU of the producer, the output gradient formed from the BatchNorm backward's operands; padding stays 0.
// Text and not a function: with the form handed over as a lambda, wino_input_k<true> came out with two instructions in another order.
#define SSV_WINO_LOAD_PATCH(VW, P, STEP, d, x, n, i, j, H, W, C, c, FORM) \
  _Pragma("unroll") for (int a_ = 0; a_ < (P); ++a_) { \
    const int hi_ = (STEP) * (i) - 1 + a_; \
    _Pragma("unroll") for (int b_ = 0; b_ < (P); ++b_) { \
      const int wi_ = (STEP) * (j) - 1 + b_; \
      vecf<VW> v = {}; \
      if ((unsigned)hi_ < (unsigned)(H) && (unsigned)wi_ < (unsigned)(W)) { \
        const size_t off = (((size_t)(n) * (H) + hi_) * (W) + wi_) * (C) + (c); \
        v = ldv<VW>((x) + off); \
        FORM; \
      } \
      (d)[a_][b_] = v; \
    } \
  }

// the STEP x STEP output tile (i, j): rows STEP * i .. of image n, zero past the edge of the map
template <int VW, int STEP>
__device__ __forceinline__ void load_tile(vecf<VW> (&y)[STEP][STEP], const float* __restrict__ dy, int n, int i, int j, int H, int W, int K, int k) {
#pragma unroll
  for (int a = 0; a < STEP; ++a)
#pragma unroll
    for (int b = 0; b < STEP; ++b) {
      const int ho = STEP * i + a, wo = STEP * j + b;
      y[a][b] = (ho < H && wo < W) ? ldv<VW>(dy + (((size_t)n * H + ho) * W + wo) * K + k) : vecf<VW>{};
    }
}

// ---- the 1-D transforms.  F(2x2, 3x3), points {0, 1, -1, inf}: only additions and halves (exact) ----------------------------------------------------------
//   B^T = [ 1  0 -1  0 ]   G = [  1    0    0  ]   A^T = [ 1  1  1  0 ]
//         [ 0  1  1  0 ]       [ 1/2  1/2  1/2 ]         [ 0  1 -1 -1 ]
//         [ 0 -1  1  0 ]       [ 1/2 -1/2  1/2 ]
//         [ 0  1  0 -1 ]       [  0    0    1  ]
struct Bt4 {
  template <int Q, class T> static __device__ __forceinline__ T row(const T (&d)[4]) {          // row Q of B^T times d
    if constexpr (Q == 0) return d[0] - d[2]; else if constexpr (Q == 1) return d[1] + d[2]; else if constexpr (Q == 2) return d[2] - d[1]; else return d[1] - d[3];
  }
  template <class T> __device__ __forceinline__ void operator()(const T (&d)[4], T (&v)[4]) const { v[0] = row<0>(d); v[1] = row<1>(d); v[2] = row<2>(d); v[3] = row<3>(d); }
};
struct At4 { template <class T> __device__ __forceinline__ void operator()(const T (&m)[4], T (&y)[2]) const {
  y[0] = m[0] + m[1] + m[2]; y[1] = m[1] - m[2] - m[3]; } };
// A (4x2) = (A^T)^T: the weight gradient's dY transform  dM = A dY A^T
struct A4 {
  template <int Q, class T> static __device__ __forceinline__ T row(const T (&y)[2]) {
    if constexpr (Q == 0) return y[0]; else if constexpr (Q == 1) return y[0] + y[1]; else if constexpr (Q == 2) return y[0] - y[1]; else return -y[1];
  }
  template <class T> __device__ __forceinline__ void operator()(const T (&y)[2], T (&m)[4]) const { m[0] = row<0>(y); m[1] = row<1>(y); m[2] = row<2>(y); m[3] = row<3>(y); }
};
struct G4 { __device__ __forceinline__ void operator()(const float (&g)[3], float (&u)[4]) const {
  u[0] = g[0]; u[1] = 0.5f * (g[0] + g[1] + g[2]); u[2] = 0.5f * (g[0] - g[1] + g[2]); u[3] = g[2]; } };
// G^T (3x4): the filter gradient's back transform  dg = G^T dU G
struct Gt4 { __device__ __forceinline__ void operator()(const float (&u)[4], float (&r)[3]) const {
  r[0] = u[0] + 0.5f * (u[1] + u[2]); r[1] = 0.5f * (u[1] - u[2]); r[2] = 0.5f * (u[1] + u[2]) + u[3]; } };

// F(4x4, 3x3), points {0, 1, -1, 1/2, -2, inf}: B^T (6x6), G (6x3), A^T (4x6)
//   B^T = [ 1 -3/2 -2  3/2  1  0 ]   G = [   1      0      0   ]   A^T = [ 1  1  1   1    1  0 ]
//         [ 0  -1  1/2 5/2  1  0 ]       [  1/3    1/3    1/3  ]         [ 0  1 -1  1/2  -2  0 ]
//         [ 0   1 -5/2 1/2  1  0 ]       [ -1/3    1/3   -1/3  ]         [ 0  1  1  1/4   4  0 ]
//         [ 0  -2  -1   2   1  0 ]       [ -16/15 -8/15  -4/15 ]         [ 0  1 -1  1/8  -8  1 ]
//         [ 0  1/2 -1 -1/2  1  0 ]       [  1/15  -2/15   4/15 ]
//         [ 0   1 -3/2 -2  3/2 1 ]       [   0      0      1   ]
struct Bt6 { template <class T> __device__ __forceinline__ void operator()(const T (&d)[6], T (&v)[6]) const {
  v[0] = d[0] - 1.5f * d[1] - 2.f * d[2] + 1.5f * d[3] + d[4];
  v[1] = -d[1] + 0.5f * d[2] + 2.5f * d[3] + d[4];
  v[2] = d[1] - 2.5f * d[2] + 0.5f * d[3] + d[4];
  v[3] = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
  v[4] = 0.5f * d[1] - d[2] - 0.5f * d[3] + d[4];
  v[5] = d[1] - 1.5f * d[2] - 2.f * d[3] + 1.5f * d[4] + d[5]; } };
struct At6 { template <class T> __device__ __forceinline__ void operator()(const T (&m)[6], T (&y)[4]) const {
  y[0] = m[0] + m[1] + m[2] + m[3] + m[4];
  y[1] = m[1] - m[2] + 0.5f * m[3] - 2.f * m[4];
  y[2] = m[1] + m[2] + 0.25f * m[3] + 4.f * m[4];
  y[3] = m[1] - m[2] + 0.125f * m[3] - 8.f * m[4] + m[5]; } };
// A (6x4) = (A^T)^T applied to a 4-vector: the weight gradient's dY transform  dM = A dY A^T
struct A6 { template <class T> __device__ __forceinline__ void operator()(const T (&y)[4], T (&m)[6]) const {
  m[0] = y[0];
  m[1] = y[0] + y[1] + y[2] + y[3];
  m[2] = y[0] - y[1] + y[2] - y[3];
  m[3] = y[0] + 0.5f * y[1] + 0.25f * y[2] + 0.125f * y[3];
  m[4] = y[0] - 2.f * y[1] + 4.f * y[2] - 8.f * y[3];
  m[5] = y[3]; } };
struct G6 { __device__ __forceinline__ void operator()(const float (&g)[3], float (&u)[6]) const {
  u[0] = g[0];
  u[1] = (g[0] + g[1] + g[2]) * (1.f / 3.f);
  u[2] = (-g[0] + g[1] - g[2]) * (1.f / 3.f);
  u[3] = (-16.f * g[0] - 8.f * g[1] - 4.f * g[2]) * (1.f / 15.f);
  u[4] = (g[0] - 2.f * g[1] + 4.f * g[2]) * (1.f / 15.f);
  u[5] = g[2]; } };
// G^T (3x6) applied to a 6-vector: the filter gradient's back transform  dg = G^T dU G
struct Gt6 { __device__ __forceinline__ void operator()(const float (&u)[6], float (&r)[3]) const {
  r[0] = u[0] + (u[1] - u[2]) * (1.f / 3.f) + (u[4] - 16.f * u[3]) * (1.f / 15.f);
  r[1] = (u[1] + u[2]) * (1.f / 3.f) - (8.f * u[3] + 2.f * u[4]) * (1.f / 15.f);
  r[2] = (u[1] - u[2]) * (1.f / 3.f) + (4.f * u[4] - 4.f * u[3]) * (1.f / 15.f) + u[5]; } };
// the ones the kernels call in their own text; the two-sided transforms below take Bt4 / A4 / Bt6 / A6 by type
constexpr At4 at4; constexpr G4 g4; constexpr Gt4 gt4; constexpr At6 at6; constexpr G6 g6; constexpr Gt6 gt6;

// ---- columns, then rows, then store position by position: o[(a * PO + b) * ps] = (F X F^T)[a][b] for the PI x PI window of d whose corner is (r0, c0) ---------
// F is one of the 1-D transforms above, PI -> PO.  One thread = one tile x VW channels; o points at the thread's channels of position 0 and is formed, with the
// position stride ps, between the two stages.  Text and not functions: as functions the input kernels came out with another instruction selection and order
// (the compiler simplifies a function before it inlines it); expanded in place every kernel is the machine code it was.
#define SSV_WINO_COLUMNS_(VW, PI, PO, d, r0, c0, o, ps, F) \
    vecf<VW> s_[PO][PI]; \
    _Pragma("unroll") for (int b_ = 0; b_ < (PI); ++b_) { \
      vecf<VW> col_[PI], m_[PO]; \
      _Pragma("unroll") for (int a_ = 0; a_ < (PI); ++a_) col_[a_] = (d)[(r0) + a_][(c0) + b_]; \
      F()(col_, m_); \
      _Pragma("unroll") for (int a_ = 0; a_ < (PO); ++a_) s_[a_][b_] = m_[a_]; \
    } \
    const size_t ps_ = (ps); \
    float* o_ = (o)
#define SSV_WINO_TRANSFORM_STORE(VW, PI, PO, d, r0, c0, o, ps, F) do { \
    SSV_WINO_COLUMNS_(VW, PI, PO, d, r0, c0, o, ps, F); \
    _Pragma("unroll") for (int a_ = 0; a_ < (PO); ++a_) { \
      vecf<VW> m_[PO]; \
      F()(s_[a_], m_); \
      _Pragma("unroll") for (int b_ = 0; b_ < (PO); ++b_) stv<VW>(o_ + (size_t)(a_ * (PO) + b_) * ps_, m_[b_]); \
    } } while (0)
// F(2x2)'s kernels form each position where they store it (F::row<Q>): the schedule follows the text
#define SSV_WINO22_TRANSFORM_STORE(VW, PI, d, r0, c0, o, ps, F) do { \
    SSV_WINO_COLUMNS_(VW, PI, 4, d, r0, c0, o, ps, F); \
    _Pragma("unroll") for (int a_ = 0; a_ < 4; ++a_) { \
      stv<VW>(o_ + (size_t)(a_ * 4 + 0) * ps_, F::row<0>(s_[a_])); \
      stv<VW>(o_ + (size_t)(a_ * 4 + 1) * ps_, F::row<1>(s_[a_])); \
      stv<VW>(o_ + (size_t)(a_ * 4 + 2) * ps_, F::row<2>(s_[a_])); \
      stv<VW>(o_ + (size_t)(a_ * 4 + 3) * ps_, F::row<3>(s_[a_])); \
    } } while (0)

// ---- the merge tails of the output transforms: the TPP partial results per channel lane, merged in fixed order by thread ts == 0 of the lane -------------------
// statistics: (count, mean, M2) triples, the pairwise update of Chan et al.; a thread that saw no pixel (count 0) is skipped
template <int VW>
__device__ __forceinline__ void merge_stats(float (&red)[3][256 * VW], vecf<VW> mean, vecf<VW> m2, float cnt, int L, int TPP, int lc, int ts, bool kok,
                                            float* __restrict__ p0, float* __restrict__ p1, int K, int k) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < VW; ++e) { red[0][tid * VW + e] = mean[e]; red[1][tid * VW + e] = m2[e]; }
  red[2][tid * VW] = cnt;
  __syncthreads();
  if (ts == 0 && kok) {
    vecf<VW> am = mean, a2 = m2;
    float an = cnt;
    for (int q = 1; q < TPP; ++q) {
      const int o = (q * L + lc) * VW;
      const float bn = red[2][o];
      if (bn == 0.f) continue;
      const float tot = an + bn;
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const float dlt = red[0][o + e] - am[e];
        a2[e] += red[1][o + e] + dlt * dlt * (an * bn / tot);
        am[e] += dlt * (bn / tot);
      }
      an = tot;
    }
    stv<VW>(p0 + (size_t)blockIdx.x * K + k, am);
    stv<VW>(p1 + (size_t)blockIdx.x * K + k, a2);
  }
}
// the gate: the plain sums of g and g * xhat
template <int VW>
__device__ __forceinline__ void merge_sums(float (&red)[3][256 * VW], vecf<VW> s1, vecf<VW> s2, int L, int TPP, int lc, int ts, bool kok,
                                           float* __restrict__ p0, float* __restrict__ p1, int K, int k) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < VW; ++e) { red[0][tid * VW + e] = s1[e]; red[1][tid * VW + e] = s2[e]; }
  __syncthreads();
  if (ts == 0 && kok) {
    vecf<VW> a1 = s1, a2 = s2;
    for (int q = 1; q < TPP; ++q) {
      const int o = (q * L + lc) * VW;
#pragma unroll
      for (int e = 0; e < VW; ++e) { a1[e] += red[0][o + e]; a2[e] += red[1][o + e]; }
    }
    stv<VW>(p0 + (size_t)blockIdx.x * K + k, a1);
    stv<VW>(p1 + (size_t)blockIdx.x * K + k, a2);
  }
}

// ==================================================================================================================== host side
inline int wino_check_shape(int N, int H, int W, int C, const char* who) {
  SSV_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "%s: bad shape (channels %% 4 == 0 required)", who);
  SSV_REQUIRE((int64_t)N * H * W * C < (1ll << 31) * 4, "%s: tensor too large", who);
  return SSV_OK;
}

// What both output transforms ask of their arguments.  cpt: channels per thread of the kernel (the lane rule); stats_ok: the map partitions into equal groups
// (F(2x2) only: ssv_wino_stats_rows_per_group; F(4x4) always does).
inline int wino_check_output(int N, int H, int W, int K, const float* M, float* y, float* pmean, float* pm2, const ssv_bn_gate* gate, int cpt, bool stats_ok,
                             const char* who) {
  if (int rc = wino_check_shape(N, H, W, K, who)) return rc;
  SSV_REQUIRE(M && y && (((uintptr_t)M | (uintptr_t)y | (uintptr_t)pmean | (uintptr_t)pm2) & 15) == 0, "%s: null or unaligned pointer", who);
  SSV_REQUIRE((pmean == nullptr) == (pm2 == nullptr), "%s: pmean / pm2 must both be given or both NULL", who);
  SSV_REQUIRE(!(pmean && gate), "%s: statistics and gate are exclusive", who);
  SSV_REQUIRE(!pmean || stats_ok, "%s: the statistics epilogue needs whole tiles (H, W even) or one image per group (got %d x %d)", who, H, W);
  SSV_REQUIRE(K % 4 == 0 && (K / cpt <= 256 ? 256 % (K / cpt) == 0 : (K / cpt) % 256 == 0), "%s: K / %d must divide or be a multiple of 256 (got K=%d)", who, cpt, K);
  if (gate) {
    SSV_REQUIRE(gate->x && gate->mean && gate->invstd && gate->psum_g && gate->psum_gx && !gate->x2 &&
                ((gate->mask != nullptr) != (gate->scale != nullptr && gate->shift != nullptr)) && ((gate->scale == nullptr) == (gate->shift == nullptr)),
                "%s: the gate carries x, mean, invstd, psum_g, psum_gx and either the byte mask or scale + shift (no second target)", who);
  }
  return SSV_OK;
}

// The four epilogues of an output transform, KERNEL<MODE>: 3 gate from the byte mask | 2 gate from scale + shift | 1 statistics | 0 plain.  The variadic
// arguments are the kernel's own up to T; the partial targets and the gate's operands follow them.
#define SSV_WINO_MODE_LADDER(KERNEL, grid, s, gate, pmean, pm2, ...) do { \
    const float* nf_ = nullptr; \
    const uint8_t* nb_ = nullptr; \
    if (gate && gate->mask) hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, s, __VA_ARGS__, gate->psum_g, gate->psum_gx, gate->x, nf_, nf_, gate->mean, gate->invstd, gate->mask); \
    else if (gate) hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, s, __VA_ARGS__, gate->psum_g, gate->psum_gx, gate->x, gate->scale, gate->shift, gate->mean, gate->invstd, nb_); \
    else if (pmean) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, s, __VA_ARGS__, pmean, pm2, nf_, nf_, nf_, nf_, nf_, nb_); \
    else hipLaunchKernelGGL(KERNEL<0>, grid, dim3(256), 0, s, __VA_ARGS__, (float*)nullptr, (float*)nullptr, nf_, nf_, nf_, nf_, nf_, nb_); } while (0)

// The filter transform and the filter gradient of either form: one thread per (k, c), `in` -> `out` (+ the kernel's further arguments), under class cls
template <class... A>
int wino_launch_kc(const char* who, int cls, void (*kern)(int, int, const float*, float*, A...), int K, int C, const float* in, float* out, void* stream, A... more) {
  SSV_REQUIRE(K > 0 && C > 0 && in && out, "%s: bad arguments", who);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(cls, s);
  hipLaunchKernelGGL(kern, dim3((unsigned)cdiv64((int64_t)K * C, 256)), dim3(256), 0, s, K, C, in, out, more...);
  SSV_CHECK_LAUNCH(who);
  return SSV_OK;
}

}  // namespace
