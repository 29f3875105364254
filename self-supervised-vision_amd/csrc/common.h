// Shared host/device helpers for libssv_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/ssv_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- error reporting ------------------------------------------------------------------------
void ssv_set_error(const char* fmt, ...);
#define SSV_FAIL(code, ...) do { ssv_set_error(__VA_ARGS__); return (code); } while (0)
#define SSV_REQUIRE(cond, ...) do { if (!(cond)) SSV_FAIL(SSV_ERR_INVALID, __VA_ARGS__); } while (0)
#define SSV_CHECK_LAUNCH(what) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) SSV_FAIL(SSV_ERR_LAUNCH, "%s: %s", (what), hipGetErrorString(e_)); } while (0)

// ---- per-class event timing (ssv_prof_*) ---------------------------------------------------
void ssv_prof_begin(int cls, hipStream_t s);
void ssv_prof_end(int cls, hipStream_t s);
struct ProfScope {
  int cls; hipStream_t s;
  ProfScope(int c, hipStream_t st) : cls(c), s(st) { ssv_prof_begin(cls, s); }
  ~ProfScope() { ssv_prof_end(cls, s); }
};

// ---- exact unsigned division by a runtime constant (n < 2^31) ----------------------------------
struct FastDiv { uint32_t mul, shr, d; };
static inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f; f.d = d ? d : 1;
  if (f.d == 1) { f.mul = 0; f.shr = 0; return f; }
  uint32_t lg = 31 - __builtin_clz(f.d);
  if (f.d & (f.d - 1)) lg += 1;                       // ceil(log2 d)
  uint32_t p = 31 + lg;
  f.mul = (uint32_t)((((uint64_t)1 << p) + f.d - 1) / f.d);
  f.shr = p - 32;
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  return f.d == 1 ? n : (__umulhi(n, f.mul) >> f.shr);
}

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// arg-max over a wave in the library's one order: value descending, the LOWER index on equal values (the first maximum, like argmax).  STEP is one exchange
// with lane ^ o; WAVE the whole butterfly, after which all 64 lanes hold the winner.  Macros on purpose: the compiler simplifies a function's body before it
// inlines it, and every kernel that moved to a function form came out with a different instruction schedule than the loop written in place.
#define SSV_ARGMAX_FIRST_STEP(v, i, o) do { \
    const float ov_ = __shfl_xor((v), (o), 64); \
    const int oi_ = __shfl_xor((i), (o), 64); \
    if (ov_ > (v) || (ov_ == (v) && oi_ < (i))) { (v) = ov_; (i) = oi_; } } while (0)
#define SSV_WAVE_ARGMAX_FIRST(v, i) _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) SSV_ARGMAX_FIRST_STEP(v, i, o_)
// sum of sm[0 .. 255] into sm[0] by a 256-thread workgroup: a fixed tree (the order of additions is part of every caller's result).  Every thread has written
// sm[threadIdx.x] and passed a barrier before; ends with a barrier.  A macro for the reason above.
#define SSV_BLOCK_SUM_256(sm) \
  for (int o_ = 128; o_ > 0; o_ >>= 1) { if ((int)threadIdx.x < o_) (sm)[threadIdx.x] += (sm)[threadIdx.x + o_]; __syncthreads(); }

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }           // workspace sections start on 256-byte boundaries

// whether no output is an input or another output; a null output (an optional one the caller left out) is skipped
static inline bool no_alias(const void* const* out, int no, const void* const* in, int ni) {
  for (int a = 0; a < no; ++a) {
    if (!out[a]) continue;
    for (int b = 0; b < ni; ++b) if (out[a] == in[b]) return false;
    for (int b = a + 1; b < no; ++b) if (out[a] == out[b]) return false;
  }
  return true;
}

// the 1x1 "convolution" that is the GEMM Y[rows, K] = X[rows, C] W[K, C]^T (w_planes: W pre-split by ssv_split_planes, or null)
static inline ssv_conv_desc gemm_conv_desc(int rows, int C, int K, int arithmetic, const void* w_planes = nullptr) {
  ssv_conv_desc cd = {};
  cd.arithmetic = arithmetic; cd.w_planes = w_planes;
  cd.N = rows; cd.H = 1; cd.W = 1; cd.C = C; cd.K = K; cd.R = 1; cd.S = 1; cd.stride = 1; cd.pad = 0; cd.Ho = 1; cd.Wo = 1;
  return cd;
}

// ---- nn.GELU() in its erf form (networks/vit.py:38, models/dino.py:30-33) --------------------------------------------------------
// erf in ~20 VALU instructions (the libm erff costs ~50 and branches): x * P5(x^2) for |x| < 1 (relative error 2e-7), 1 - u P4(u) exp(-x^2) with
// u = 1 / (1 + 0.932 |x|) beyond (Abramowitz-Stegun 7.1.26's form, coefficients re-fitted: 5e-10 in exact arithmetic); 1.3e-7 absolute in fp32 over
// all x (tools/probe/fast_erf_check.py) - the rounding class of 0.5 * v * (1 + erf(.)) whatever erf is used.  Every GELU of the library - the
// stand-alone kernels of vit.hip and the GEMM epilogues of conv_mfma.hip - goes through these, so fused and unfused forms agree bit for bit.
__device__ __forceinline__ float ssv_erf(float x) {
  const float z = x * x, t = __builtin_fabsf(x);
  float a = -0.0005631421809084713f;
  a = __builtin_fmaf(a, z, 0.004917551297694445f);
  a = __builtin_fmaf(a, z, -0.02671131119132042f);
  a = __builtin_fmaf(a, z, 0.11280179768800735f);
  a = __builtin_fmaf(a, z, -0.37612324953079224f);
  a = __builtin_fmaf(a, z, 1.1283791065216064f);
  a *= x;
  const float u = __builtin_amdgcn_rcpf(__builtin_fmaf(0.932012140750885f, t, 1.f));
  float b = 0.3885830342769623f;
  b = __builtin_fmaf(b, u, -0.9805029630661011f);
  b = __builtin_fmaf(b, u, 0.5967519283294678f);
  b = __builtin_fmaf(b, u, 0.47274520993232727f);
  b = __builtin_fmaf(b, u, 0.529606282711029f);
  const float e = __builtin_amdgcn_exp2f(z * -1.4426950408889634f);
  b = __builtin_fmaf(-(b * u), e, 1.f);
  return t < 1.f ? a : __builtin_copysignf(b, x);
}
// standard normal cdf and pdf at v
__device__ __forceinline__ float ssv_norm_cdf(float v) { return 0.5f * (1.f + ssv_erf(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float ssv_norm_pdf(float v) { return 0.39894228040143267794f * __builtin_amdgcn_exp2f(v * v * -0.72134752044448170368f); }
__device__ __forceinline__ float ssv_gelu(float v) { return 0.5f * v * (1.f + ssv_erf(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float ssv_gelu_grad(float v) { return ssv_norm_cdf(v) + v * ssv_norm_pdf(v); }
