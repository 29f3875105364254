// What the five attention kernels of csrc/vit.hip share, written once (tiling: see the head of vit.hip).  Included by that file only.
//   functions  row32 (a 32-float row fragment, global or LDS), head_row / stat_base (the per-(image, head) pointers), Walk (a thread's float4s of a staged
//              32 x 64 tile) under Stage<NW> and every other staging site, store_tile_T / store_tile_T_rows (the output tiles)
//   text       SSV_ATTN_WAVE_TILE (the wave's coordinates), SSV_ATTN_STREAM_BEGIN / _END (the double-buffered loop), SSV_ATTN_PROD32 (the 32-step fp32 MFMA
//              product), SSV_ATTN_SOFTMAX_STEP (the online softmax step), SSV_ATTN_P_DS (P and dS from S and dP), SSV_ATTN_ACC_T + SSV_ATTN_ACC_PAIR (the
//              transposed accumulation, one or two pairs), SSV_ATTN_STORE_O_LSE (the forward's epilogue).  The text pieces name the locals SSV_ATTN_WAVE_TILE declares.
// Every kernel is, instruction for instruction, the machine code it was when each carried its own copy of these lines (tools/isa_compare.py,
// profiles/attn_once_isa_vs_parent.json); where that needed text instead of a function, the comment at the macro says what the function form changed.
#pragma once
#include "common.h"
#include "split_bf16.h"

namespace {

constexpr int DH = 64;

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
using splitbf::acc32_row;

// 32 consecutive floats of one row (global memory, or a staged tile's) -> registers, optionally scaled
__device__ __forceinline__ void row32(const float* __restrict__ p, float* __restrict__ r, float scale = 1.f) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f32x4 v = *(const f32x4*)(p + 4 * i);
    r[4 * i + 0] = v[0] * scale; r[4 * i + 1] = v[1] * scale; r[4 * i + 2] = v[2] * scale; r[4 * i + 3] = v[3] * scale;
  }
}

// acc^T[d][col] tile stored as rows of a [T][ld] matrix: lane (col, half) owns 4 consecutive d per register quad
__device__ __forceinline__ void store_tile_T(float* __restrict__ base, int64_t row_stride, int row, bool valid, int half,
                                             const f32x16& lo, const f32x16& hi, float mul) {
  if (!valid) return;
  float* p = base + (int64_t)row * row_stride;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = lo[4 * jj + e] * mul; b[e] = hi[4 * jj + e] * mul; }
    *(f32x4*)(p + 8 * jj + 4 * half) = a;
    *(f32x4*)(p + 32 + 8 * jj + 4 * half) = b;
  }
}

// The same tile through a wave-private 32 x 64 float LDS scratch, so that the global stores are whole 256-byte rows (16 lanes x 16 bytes, four rows per
// instruction) instead of 64 scattered 16-byte pieces: the scattered form is store-ISSUE bound (~7 B / cycle / CU: round 4's cycle stamps found the 37-token
// backward spending a quarter of its time issuing dQ stores).  Row c keeps its sixteen 16-byte slots XOR-swizzled with c & 15: the transposing writes and the
// row-major reads are both free of bank conflicts without padding (the scratch is exactly one tile).  Rows [0, nrows) of the tile are stored.
__device__ __forceinline__ void store_tile_T_rows(float* __restrict__ scratch, float* __restrict__ base, int64_t row_stride, int row0, int nrows, int lane,
                                                  const f32x16& lo, const f32x16& hi, float mul) {
  const int c = lane & 31, half = lane >> 5;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = lo[4 * jj + e] * mul; b[e] = hi[4 * jj + e] * mul; }
    *(f32x4*)(scratch + c * 64 + (((2 * jj + half) ^ (c & 15)) << 2)) = a;
    *(f32x4*)(scratch + c * 64 + (((8 + 2 * jj + half) ^ (c & 15)) << 2)) = b;
  }
  const int s = lane & 15;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = 4 * k + (lane >> 4);
    const f32x4 v = *(const f32x4*)(scratch + r * 64 + ((s ^ (r & 15)) << 2));
    if (r < nrows) *(f32x4*)(base + (int64_t)(row0 + r) * row_stride + 4 * s) = v;
  }
}

// A workgroup = NW wavefronts = NW consecutive 32-row tiles of ONE (image, head).  The tiles it streams over (keys/values in the
// forward and dQ passes, queries/dO in the dK/dV pass) are staged once per workgroup into LDS with coalesced 16-byte loads
// (row stride 68 floats: conflict-free ds_read_b128 of a 32-float row fragment) and double-buffered: the global loads of tile
// t+1 are in flight while the MFMAs of tile t run.
// Scores are kept in log2 units (Q is pre-multiplied by scale * log2 e), so every softmax exponential is one v_exp_f32;
// the saved log-sum-exp stays in natural units (converted on store / load).
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr int TS = 68;                                        // LDS row stride (floats) of a staged 32 x 64 tile

// Where a wavefront stands, as locals of the kernel: lane, wave, the lane's column c of a 32 x 32 accumulator and its half of the head dimension, the first row r0
// of the wave's 32-row tile TILE (an expression over wave) of image b and head h, whether that tile lies inside the sequence (a trailing wave only helps
// staging), the image's first token and the lane's own row clamped into the sequence.  Text and not a struct: as members of a struct built by a forced-inline constructor (in this
// order, and with the rest computed at its use) attn_fwd_k<2, 4> gained 1 instruction - also when only attn_fwd_sp_k used the struct.
#define SSV_ATTN_WAVE_TILE(r0, row, TILE, T) \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5; \
  const int r0 = (TILE) * 32, h = blockIdx.y, b = blockIdx.z; \
  const bool active = r0 < (T); \
  const int64_t tok0 = (int64_t)b * (T); \
  const int row = min(r0 + c, (T) - 1);
// row `row` (counted from the batch's first token) of head h's 64 columns in a [tokens][ld] matrix; the first entry of an (image, head)'s LSE / DELTA
template <class F> __device__ __forceinline__ F* head_row(F* p, int64_t row, int ld, int h) { return p + row * ld + h * DH; }
__device__ __forceinline__ int64_t stat_base(int b, int heads, int h, int T) { return ((int64_t)b * heads + h) * T; }

// float4 i of this thread's share of a 32 x 64 tile staged by NW * 64 threads: tile row r, float4 q of the 16 in the row
template <int NW>
struct Walk {
  int r, q;
  __device__ __forceinline__ explicit Walk(int i) { const int e = i * NW * 64 + threadIdx.x; r = e >> 4; q = e & 15; }
  __device__ __forceinline__ int c4() const { return q * 4; }
  __device__ __forceinline__ int64_t row(int row0, int T) const { return min(row0 + r, T - 1); }      // rows past the sequence repeat its last row
};

template <int NW>
struct Stage {                                                // registers holding one thread's share of two 32x64 tiles
  static constexpr int N4 = 512 / (NW * 64);                  // float4 per thread per tile
  f32x4 a[N4], b[N4];
  __device__ __forceinline__ void load(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, int row0, int T) {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const Walk<NW> w(i);
      const int64_t row = w.row(row0, T);
      a[i] = *(const f32x4*)(A + row * lda + w.c4());
      b[i] = *(const f32x4*)(B + row * ldb + w.c4());
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ sa, float* __restrict__ sb) const {
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const Walk<NW> w(i);
      *(f32x4*)(sa + w.r * TS + w.c4()) = a[i];
      *(f32x4*)(sb + w.r * TS + w.c4()) = b[i];
    }
  }
};

// The double-buffered walk over the 32-row tiles of the sequence: load(t0) fetches the tile that starts at row t0 into registers, store(stage) writes those
// registers to LDS stage `stage` (two lambdas of the kernel); between BEGIN and END stands the work on tile t0 in stage buf, under which the loads of tile
// t0 + 32 fly.  Text and not a function: with the work handed over as a third lambda attn_bwd_dq_k gained 2 instructions.  (attn_fwd_k's two lambdas capture
// its pointers by value: capturing them by reference cost that kernel 2 instructions.)
#define SSV_ATTN_STREAM_BEGIN(T, t0, buf, load, store) \
  load(0); \
  store(0); \
  __syncthreads(); \
  int buf = 0; \
  for (int t0 = 0; t0 < (T); t0 += 32, buf ^= 1) { \
    const bool more_ = t0 + 32 < (T); \
    if (more_) load(t0 + 32);
#define SSV_ATTN_STREAM_END(buf, store) \
    if (more_) store(buf ^ 1); \
    __syncthreads(); \
  }

// The 32 x 32 product over one half of the head dimension, 32 steps of v_mfma_f32_32x32x2_f32: acc[row of a][column of b] += sum_i (a[i] A_MUL) b[i]; A_MUL is
// empty or `* factor`.  Text and not a function: taking the fragments as array references or pointers and the accumulator by value, attn_bwd_dq_k gained 2 instructions.
#define SSV_ATTN_PROD32(acc, a, A_MUL, b) \
  _Pragma("unroll") for (int i_ = 0; i_ < 32; ++i_) acc = __builtin_amdgcn_mfma_f32_32x32x2f32((a)[i_] A_MUL, (b)[i_], acc, 0, 0, 0);

// One step of the online softmax over the 32 keys t0.. of S^T (query on the lane): keys past T masked, running maximum m and sum l updated, s becomes P^T and the
// output accumulators are rescaled.  Text and not a function: with s, m, l, o_lo, o_hi by reference all four forward kernels came out in another instruction
// order (attn_fwd_k<4>: 886 -> 887 instructions).
#define SSV_ATTN_SOFTMAX_STEP(s, t0, T, half, m, l, o_lo, o_hi) { \
    float mt_ = -INFINITY; \
    _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) { \
      if ((t0) + acc32_row(j_, half) >= (T)) (s)[j_] = -INFINITY; \
      mt_ = fmaxf(mt_, (s)[j_]); \
    } \
    mt_ = fmaxf(mt_, __shfl_xor(mt_, 32, 64)); \
    const float mn_ = fmaxf(m, mt_); \
    const float alpha_ = ex2((m) - mn_);                      /* m = -inf on the first tile -> 0 */ \
    float ls_ = 0.f; \
    _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) { (s)[j_] = ex2((s)[j_] - mn_); ls_ += (s)[j_]; } \
    ls_ += __shfl_xor(ls_, 32, 64); \
    l = (l) * alpha_ + ls_; \
    m = mn_; \
    _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) { (o_lo)[j_] *= alpha_; (o_hi)[j_] *= alpha_; } \
  }

// P = exp2(S - lse) (0 where the (query, key) pair is padding) and dS = P (dP - delta) of accumulator register j: s[j] becomes P, dp[j] becomes dS.
// Text and not a function: as a function over (s, dp, j, live, lse, delta) attn_bwd_dq_k was unchanged, attn_bwd_dkv_k<4> went from 1086 to 1038 instructions.
#define SSV_ATTN_P_DS(s, dp, j, live, lse, delta) { \
    const float p_ = (live) ? ex2((s)[j] - (lse)) : 0.f; \
    (s)[j] = p_; \
    (dp)[j] = p_ * ((dp)[j] - (delta)); \
  }

// The transposed accumulation over the 16 register steps of x (step j = tile rows acc32_row(j, half) of the 32-row tile that starts at sequence row t0):
// lo / hi += rows[c], rows[32 + c] x x[j] for every PAIR; a step whose two rows are both past T is skipped (wave-uniform: x is 0 there).
// Text and not a function: with the tile pointer, the accumulators and x by reference attn_fwd_k and attn_bwd_dq_k gained 3-4 instructions, attn_bwd_fused_k 2.
#define SSV_ATTN_ACC_PAIR(rows, ROW0_PLUS, x, lo, hi) { \
    const float* r_ = (rows) + (ROW0_PLUS acc32_row(j_, half)) * TS; \
    lo = __builtin_amdgcn_mfma_f32_32x32x2f32(r_[c], (x)[j_], lo, 0, 0, 0); \
    hi = __builtin_amdgcn_mfma_f32_32x32x2f32(r_[32 + c], (x)[j_], hi, 0, 0, 0); \
  }
#define SSV_ATTN_ACC_T(t0, T, PAIRS) \
  _Pragma("unroll") for (int j_ = 0; j_ < 16; ++j_) { \
    if ((t0) + acc32_row(j_, 0) >= (T)) continue; \
    PAIRS \
  }

// The forward's epilogue: the wave's output tile, divided by the softmax sum, through its 32 x 64 LDS scratch (whole rows to global memory) and the log-sum-exp.
// Text and not a function: as a function both forward kernels kept their instruction count in another order.
#define SSV_ATTN_STORE_O_LSE(scratch, O, ldo, LSE, q0, T, heads, o_lo, o_hi, m, l) \
  const bool valid = q0 + c < (T); \
  if (active) store_tile_T_rows((scratch) + wave * 2048, head_row(O, tok0, ldo, h), ldo, q0, min(32, (T) - q0), lane, o_lo, o_hi, 1.f / (l)); \
  if (valid && half == 0) LSE[stat_base(b, heads, h, T) + q0 + c] = ((m) + log2f(l)) * LN2;

}  // namespace
