// What the row-streaming kernels of csrc/bn.hip and csrc/pool.hip share, written once.  Included by those two files only.
//   functions  ld4 / st4 / fma4, st_partial, fin_lane / fin_group_sum / fin_put / fin_sum (the finalize kernels' group prologue and LDS merge), bn_bwd_acc / bn_bwd_dx
//              (the BatchNorm-backward row), pool_decode, window_scan and argmax_gather (MaxPool2d(3, 2, 1) forward and backward)
//   text       SSV_ROW_LANE / SSV_ROW_LANE_OR_RETURN (a lane's coordinates and row range), SSV_WALK4 (four rows in flight), SSV_BLOCK_TAIL / SSV_BLOCK_TAIL2
// Every kernel but maxpool_bwd_k is, instruction for instruction, the machine code it was when each carried its own copy of these lines (tools/isa_compare.py,
// profiles/bn_once_isa_vs_parent.json); where that needed text instead of a function, the comment at the macro says what the function form changed.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
  f32x4 r;
  r[0] = __builtin_fmaf(a[0], b[0], c[0]); r[1] = __builtin_fmaf(a[1], b[1], c[1]);
  r[2] = __builtin_fmaf(a[2], b[2], c[2]); r[3] = __builtin_fmaf(a[3], b[3], c[3]);
  return r;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------------
// A 256-thread block is CT channel groups (one float4 each) x RT row lanes; block (bx, by) owns rows [r0, r1) of the channel groups by * CT ...  Declares tid, ct,
// rt, c4, r0, r1 and `active`, or returns on an idle lane.  Text: as a function returning a struct, left with `if (!l.active) return;`, every bn_apply_k and
// bn_bwd_apply_k came out 2 instructions longer (bn_apply_k<false, 0>: 185 -> 187) - the test on the bool is not the branch the `||` form makes.
#define SSV_ROW_LANE_(M, CT, rpb, LIVE) \
  const int tid = threadIdx.x; \
  const int ct = tid % (CT), rt = tid / (CT); \
  const int c4 = blockIdx.y * (CT) + ct; \
  LIVE; \
  const int64_t r0 = (int64_t)blockIdx.x * (rpb); \
  const int64_t r1 = r0 + (rpb) < (M) ? r0 + (rpb) : (M)
#define SSV_ROW_LANE(M, C, CT, RT, rpb) SSV_ROW_LANE_(M, CT, rpb, const bool active = rt < (RT) && c4 < (C) / 4)
#define SSV_ROW_LANE_OR_RETURN(M, C, CT, RT, rpb) SSV_ROW_LANE_(M, CT, rpb, if (rt >= (RT) || c4 >= (C) / 4) return)

#define SSV_WALK4(start, r1, RT, body) \
  { int64_t r_ = (start); \
    for (; r_ + 3 * (RT) < (r1); r_ += 4 * (RT)) { body(r_); body(r_ + (RT)); body(r_ + 2 * (RT)); body(r_ + 3 * (RT)); } \
    for (; r_ < (r1); r_ += (RT)) body(r_); }

// The block tail: every lane's sums to LDS, the rt == 0 lanes add the other RT - 1 in the order j = 1 .. RT - 1 (part of every result) and run the statements
// that follow.  Text: as a function (returning whether the lane folds, or taking the rest as a lambda) colsum_partial_k and bn_bwd_reduce_k<0 / 1> were
// reordered, bn_bwd_reduce_k<2> went 464 -> 463 and bn_pool_bwd_k<false> 1818 -> 1819.
#define SSV_BLOCK_TAIL(CT, RT, sm1, s1, ...) \
  sm1[tid] = s1; \
  __syncthreads(); \
  if (active && rt == 0) { \
    for (int j = 1; j < (RT); ++j) s1 += sm1[j * (CT) + ct]; \
    __VA_ARGS__ \
  }
#define SSV_BLOCK_TAIL2(CT, RT, sm1, sm2, s1, s2, ...) \
  sm1[tid] = s1; sm2[tid] = s2; \
  __syncthreads(); \
  if (active && rt == 0) { \
    for (int j = 1; j < (RT); ++j) { s1 += sm1[j * (CT) + ct]; s2 += sm2[j * (CT) + ct]; } \
    __VA_ARGS__ \
  }
__device__ __forceinline__ void st_partial(float* __restrict__ p, int c4, int C, f32x4 v) { st4(p + (size_t)blockIdx.x * C + 4 * c4, v); }

// ---- finalize: FIN_C channels x FIN_G groups of partial blocks per workgroup, so that even the narrowest layer (C = 64) gets 8 workgroups and a lane walks only
// nblk / 32 partials (4 loads in flight); the groups' sums meet in LDS and are added in the order 0 .. FIN_G - 1
constexpr int FIN_C = 8, FIN_G = 32;

struct FinLane { int cl, grp, c; bool ok; int b0, b1; };
__device__ __forceinline__ FinLane fin_lane(int C, int nblk) {
  FinLane f;
  f.cl = threadIdx.x % FIN_C; f.grp = threadIdx.x / FIN_C;
  f.c = blockIdx.x * FIN_C + f.cl;
  f.ok = f.c < C;
  const int per = (nblk + FIN_G - 1) / FIN_G;
  f.b0 = min(f.grp * per, nblk); f.b1 = min(f.b0 + per, nblk);
  return f;
}

template <class F>
__device__ __forceinline__ double fin_group_sum(int b0, int b1, F&& term) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int b = b0;
  for (; b + 3 < b1; b += 4) { a0 += term(b); a1 += term(b + 1); a2 += term(b + 2); a3 += term(b + 3); }
  for (; b < b1; ++b) a0 += term(b);
  return (a0 + a1) + (a2 + a3);
}

__device__ __forceinline__ void fin_put(double (*sm)[FIN_C], const FinLane& f, double v) { sm[f.grp][f.cl] = v; }
__device__ __forceinline__ double fin_sum(const double (*sm)[FIN_C], const FinLane& f) {
  double s = 0.0;
  for (int g = 0; g < FIN_G; ++g) s += sm[g][f.cl];
  return s;
}
__device__ __forceinline__ void fin_sum(const double (*sm1)[FIN_C], const double (*sm2)[FIN_C], const FinLane& f, double& a, double& b) {
  a = 0.0; b = 0.0;
  for (int g = 0; g < FIN_G; ++g) { a += sm1[g][f.cl]; b += sm2[g][f.cl]; }
}

// ---- the BatchNorm-backward row, accumulating and storing: the plain kernels and the image stem's pooled forms run the same lines ---------------------------
__device__ __forceinline__ void bn_bwd_acc(f32x4 g, f32x4 xv, f32x4 mu, f32x4 is, f32x4& s1, f32x4& s2) {
  const f32x4 xh = (xv - mu) * is;
  s1 += g; s2 += g * xh;
}
__device__ __forceinline__ void bn_bwd_dx(float* __restrict__ dx, f32x4 g, f32x4 xv, f32x4 mu, f32x4 is, f32x4 gi, f32x4 a1, f32x4 a2) {
  const f32x4 xh = (xv - mu) * is;
  st4(dx, gi * (g - a1 - xh * a2));
}

// ---- MaxPool2d(kernel 3, stride 2, pad 1) in NHWC ----------------------------------------------------------------------------------------
// float4 group i of an [N][Hy][Wx][C4] map
struct PoolIdx { int c4, w, h, n; };
__device__ __forceinline__ PoolIdx pool_decode(int64_t i, int C4, int Wx, int Hy) {
  const int64_t t = i / C4, u = t / Wx;
  return {(int)(i % C4), (int)(t % Wx), (int)(u % Hy), (int)(u / Hy)};
}

// The window of output pixel p, scanned r-major over f(raw): a strictly greater value (or a NaN) replaces the running max, so ties resolve to the first element
// like ATen.  best = the max of f, raw = the loaded value at the arg-max pixel, slot = r * 3 + s (0 .. 8) per element.
struct PoolMax { f32x4 best, raw; uchar4 slot; };
template <bool RAW, class F>
__device__ __forceinline__ PoolMax window_scan(const PoolIdx& p, int H, int W, int C, const float* __restrict__ x, F&& f) {
  f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  f32x4 braw = {0.f, 0.f, 0.f, 0.f};
  int bi[4] = {0, 0, 0, 0};
  bool first[4] = {true, true, true, true};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int hi = p.h * 2 - 1 + r;
    if ((unsigned)hi >= (unsigned)H) continue;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int wi = p.w * 2 - 1 + s;
      if ((unsigned)wi >= (unsigned)W) continue;
      const f32x4 raw = ld4(x + (((size_t)p.n * H + hi) * W + wi) * C + 4 * p.c4);
      const f32x4 v = f(raw);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (first[e] || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; if constexpr (RAW) braw[e] = raw[e]; bi[e] = r * 3 + s; first[e] = false; }
    }
  }
  return {best, braw, make_uchar4((uint8_t)bi[0], (uint8_t)bi[1], (uint8_t)bi[2], (uint8_t)bi[3])};
}

// Gather form of the backward (no atomics, deterministic): the sum of dy over the windows whose arg-max slot points back at input pixel (n, hi, wi).  A pixel sits
// in at most 2 x 2 windows: along each axis the window (c + 1) >> 1 with slot (c + 1) & 1, and for odd c also the window before it with slot 2.  The four
// candidates are visited slot-row major.
__device__ __forceinline__ f32x4 argmax_gather(int n, int hi, int wi, int Ho, int Wo, int C4, int c4, const float* __restrict__ dy, const uint8_t* __restrict__ am) {
  const int hA = (hi + 1) >> 1, rA = (hi + 1) & 1, wA = (wi + 1) >> 1, sA = (wi + 1) & 1;
  // (window, slot) per axis in increasing slot order: [A (slot 0/1)], then [A - 1 (slot 2)] when the coordinate is odd
  const int hw[2] = {hA, hA - 1}, hs[2] = {rA, 2}, ww[2] = {wA, wA - 1}, wsl[2] = {sA, 2};
  const bool hv[2] = {hA < Ho, (hi & 1) != 0}, wv[2] = {wA < Wo, (wi & 1) != 0};
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (hv[i] && wv[j]) {
        const size_t o = (((size_t)n * Ho + hw[i]) * Wo + ww[j]) * C4 + c4;
        const uchar4 m = reinterpret_cast<const uchar4*>(am)[o];
        const f32x4 d = ld4(dy + o * 4);
        const int slot = hs[i] * 3 + wsl[j];
        g[0] += m.x == slot ? d[0] : 0.f; g[1] += m.y == slot ? d[1] : 0.f;
        g[2] += m.z == slot ? d[2] : 0.f; g[3] += m.w == slot ? d[3] : 0.f;
      }
    }
  return g;
}

}  // namespace
