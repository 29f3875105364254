// "Queries against a bank", written once: what the nearest-neighbour lookup (nnlookup.hip), ProtoNCE (protonce.hip) and the queue InfoNCE (densecl.hip) share.
//   * scalar helpers: mul_rn, LOG2E, arith_ok, vt_off;
//   * prep_planes: the queries' three bf16 planes in fragment order, the body of nn_prep_k, pn_prep_k and qn_prep_k;
//   * pad_rows: a zero-padded copy of bank rows, the body of pn_pad_k and qn_pad_k;
//   * the flash-forward-shaped pass over one slice of bank rows, the body of pn_fused_k and qn_fused_k: the text of bank_softmax_pass.h, included in both.
//     Its operand plan and numerics are described in protonce.hip; what the two families do differently is a compile-time description of the source
//     (Segments, Range) taken by `if constexpr`, so each instantiation holds its family's expressions and nothing of the other's;
//   * host side: the fields and rules of a fused plan, the chunk rule of the unfused route, the <DT, KT> launch ladder.
// The kernels stay in their files under their names: the profiler's classes, DESIGN.md and the tests name them.
#pragma once
#include "common.h"
#include "split_bf16.h"
#include <math.h>

namespace banksm {

constexpr float LOG2E = 1.4426950408889634f;

// one fp32 multiply that stays one whatever the contraction default: where a kernel wants the exact product inside a subtraction it writes the fma itself
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

inline bool arith_ok(int32_t a) { return a == SSV_ARITH_F32_MFMA || a == SSV_ARITH_BF16X3; }

// float offset of column `col` of row `row` in a wave's tile of bank rows [32][D]: the 16-byte granules of a row are XOR-ed with the row's low three
// bits, so the 32 lanes that write one granule column of 32 rows spread over 8 granules, and the 32 lanes that read 32 consecutive columns of ONE row still
// touch 32 distinct banks (the XOR permutes granules inside an aligned group of 8 = 32 floats)
template <int D>
__device__ __forceinline__ int vt_off(int row, int col) { return row * D + ((((col >> 2) ^ (row & 7)) << 2) | (col & 3)); }

// ---- the queries' planes -----------------------------------------------------------------------------------------------------------------------------------
// m rows of width d into three bf16 planes in fragment order with NS slabs of 16 columns: the 16 bytes lane l needs for (plane, slab, tile of 32 queries) sit
// at ((plane * NS + slab) * T + tile) * 64 + l (one (slab, tile) per wave); rows behind m and columns behind d are zeros.  COLS: there may be columns behind d
// (the lookup rounds its slabs up to a multiple of four); without it 16 NS == d and the two column guards are not compiled
template <bool COLS>
__device__ __forceinline__ void prep_planes(int d, int m, int T, int NS, const float* __restrict__ q, u32x4* __restrict__ planes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nfrag = NS * T;
  const int u = blockIdx.x * 4 + wave;
  if (u >= nfrag) return;
  const int s = u / T, t = u % T, i = 32 * t + (lane & 31), col = 16 * s + 8 * (lane >> 5);
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
  if (i < m) {
    const float* p = q + (int64_t)i * d + col;
    if (!COLS || col < d) a = *(const f32x4*)p;
    if (!COLS || col + 4 < d) b = *(const f32x4*)(p + 4);
  }
  bf16x8 pl[3];
  splitbf::split8(a, b, pl);
#pragma unroll
  for (int k = 0; k < 3; ++k) planes[((int64_t)k * nfrag + u) * 64 + lane] = __builtin_bit_cast(u32x4, pl[k]);
}

// ---- the padded bank of the unfused route --------------------------------------------------------------------------------------------------------------------
// rows [0, k) of src into dst [kp][4 d4], zero rows behind k (the data-gradient GEMM contracts whole 16-row groups)
__device__ __forceinline__ void pad_rows(int64_t k, int64_t kp, int d4, const f32x4* __restrict__ src, f32x4* __restrict__ dst) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= kp * d4) return;
  dst[u] = u < k * d4 ? src[u] : f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- the fused pass ------------------------------------------------------------------------------------------------------------------------------------------
// The pass itself is the text of bank_softmax_pass.h, included inside pn_fused_k and qn_fused_k.  What the two families do differently is this compile-time
// description of the source, which the text takes by `if constexpr`; a family leaves the other's fields null.
template <bool PER_ROW_>
struct Source {
  static constexpr bool PER_ROW = PER_ROW_;
  // PER_ROW (ProtoNCE, one segment of prototypes): a scale per bank row, V = inv_phi o C, the positive lies in the bank and its score is caught on the way
  const float* inv_phi;                 // the scale of every bank row
  const int32_t* labels;                // [segs][m] the positive of every query, counted from its segment's first row
  float* spos;                          // [segs][mpad] the positive's score
  int seg; int64_t seg_b; int m;        // the slice's segment, its first row (its end is the pass's `end`), the queries
  // otherwise (queue InfoNCE, rows [0, end)): one scalar scale, V = the bare rows, no positive inside the bank
  float inv_temp;
};
using Segments = Source<true>;
using Range = Source<false>;

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------
struct FusedPlan {                                    // what every plan of a fused pass holds
  int T, mpad, KT, DT;                                // tiles of 32 queries, queries with the pad of the last tile, query tiles of a workgroup, d / 32
  size_t pm_bytes, pacc_bytes, planes_bytes;          // the partials' maxima (and, as many again, sums), their accumulators, the queries' planes
};
inline void plan_tiles(FusedPlan& p, int32_t m, int32_t d) {
  p.T = cdiv(m, 32); p.mpad = p.T * 32; p.DT = d / 32;
  p.KT = (p.T == 1 || p.DT >= 3) ? 1 : 2;             // two query tiles at d >= 96 do not fit the register file (the compiler's report: spills)
}
inline void plan_bytes(FusedPlan& p, int64_t slices, int32_t d) {      // four partials per slice
  p.pm_bytes = up256((size_t)4 * slices * p.mpad * 4);
  p.pacc_bytes = up256((size_t)4 * slices * p.mpad * d * 4);
  p.planes_bytes = (size_t)3 * (d / 16) * p.T * 1024;
}

// the unfused route takes the queries in chunks of S [cr][kp] against the kp rows of the padded bank
constexpr int CHUNK_ROWS = 1024;                      // query rows of one chunk of S
constexpr int64_t CHUNK_ELEMS = 1ll << 25;            // ... and its elements: fewer rows against a long bank
inline int chunk_rows(int64_t kp, int32_t m) {
  int64_t cr = CHUNK_ELEMS / kp;
  if (cr > CHUNK_ROWS) cr = CHUNK_ROWS;
  if (cr > m) cr = m;
  if (cr < 1) cr = 1;
  return (int)cr;
}

// launches KERNEL<DT, KT> at the plan's pair: <4, 1> <3, 1> <2, 1 | 2> <1, 1 | 2>
#define SSV_FUSED_LADDER(KERNEL, p, grid, stream, ...) do { \
    if ((p).DT == 4) hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if ((p).DT == 3) hipLaunchKernelGGL((KERNEL<3, 1>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if ((p).DT == 2 && (p).KT == 1) hipLaunchKernelGGL((KERNEL<2, 1>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if ((p).DT == 2) hipLaunchKernelGGL((KERNEL<2, 2>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else if ((p).KT == 1) hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(256), 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<1, 2>), grid, dim3(256), 0, stream, __VA_ARGS__); } while (0)

}  // namespace banksm
