// The fused bank-softmax pass, as TEXT: the body of pn_fused_k (csrc/protonce.hip) and of qn_fused_k (csrc/densecl.hip) from behind their prologues to their end,
// included inside each of the two kernels and nowhere else.  Text and not a function on purpose: the compiler simplifies a function before it inlines it, and
// the function form of this pass came out with another instruction schedule that measured 0.5 % slower in qn_fused_k<4, 1>.  Expanded in place, every
// instantiation is, instruction for instruction, the machine code the kernels had when each carried its own copy of this text (tools/isa_compare.py).
// The including kernel (a template over DT and KT, 256 threads) has in scope:
//   SRC, src         banksm::Segments or banksm::Range (csrc/bank_softmax.h) and its value: what the two families do differently, taken by `if constexpr`
//   D, vt            32 * DT and __shared__ float vt[4][32 * D], the waves' tiles of V
//   lane, wave, c, half, sl, tb     the thread's place; the slice (the index of its partials) and the first query tile of the workgroup
//   bank, end, L     the bank rows, the row behind the last one of the range, rows of one slice
//   slice0()         the slice's first row: a lambda, so that it is computed where each kernel's own body computed it - as a value formed in the prologue it
//                    moved two instructions there
//   T, mpad, planes, pm, pl, pacc   as the kernels' parameters
// The operand plan and the numerics are described at the head of csrc/protonce.hip.
  constexpr int NS = 2 * DT;
  const int64_t nfrag = (int64_t)NS * T;
  int tt[KT];                                                           // tiles behind the last repeat it (their results are not written)
  [[maybe_unused]] int labg[KT];                                        // Segments: the bank row of the query's positive
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    tt[t] = min(tb + t, T - 1);
    if constexpr (SRC::PER_ROW) {
      const int i = 32 * tt[t] + c;
      const int lab = i < src.m ? src.labels[(int64_t)src.seg * src.m + i] : -1;
      labg[t] = (unsigned)lab < (unsigned)(end - src.seg_b) ? (int)src.seg_b + lab : -1;       // a label outside the segment matches no row (pn_check_k reports it)
    }
  }
  auto frag = [&](int s, int t, int q) { return __builtin_bit_cast(bf16x8, planes[(q * nfrag + (int64_t)s * T + tt[t]) * 64 + lane]); };
  float mrun[KT], lrun[KT];
  f32x16 out[KT][DT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    mrun[t] = -INFINITY; lrun[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[t][dt][r] = 0.f;
  }
  float* myv = vt[wave];
  // the wave's quarter of the slice, 32 bank rows at a time (bounds are uniform over the wave: the matrix instructions run with all lanes)
  const int64_t q0 = slice0() + (int64_t)wave * (L >> 2);
  const int64_t q1 = q0 + (L >> 2) < end ? q0 + (L >> 2) : end;
  for (int64_t r0 = q0; r0 < q1; r0 += 32) {
    const int64_t brow = r0 + c < end ? r0 + c : end - 1;               // rows behind the end repeat the last one and are masked by index below
    const float* bp = bank + brow * D + 8 * half;
    [[maybe_unused]] float ipr = 0.f;
    if constexpr (SRC::PER_ROW) ipr = src.inv_phi[brow];
    f32x16 acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    __builtin_amdgcn_wave_barrier();                                    // the previous tile's transposed reads are behind this tile's writes
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const f32x4 a = *(const f32x4*)(bp + 16 * s), b = *(const f32x4*)(bp + 16 * s + 4);
      bf16x8 xb[3];
      splitbf::split8(a, b, xb);
      if constexpr (SRC::PER_ROW) {
        *(f32x4*)(myv + banksm::vt_off<D>(c, 16 * s + 8 * half)) = a * ipr;      // V = inv_phi o C: one fp32 multiply, the one pn_fold_k repeats for the positive's row
        *(f32x4*)(myv + banksm::vt_off<D>(c, 16 * s + 8 * half + 4)) = b * ipr;
      } else {
        *(f32x4*)(myv + banksm::vt_off<D>(c, 16 * s + 8 * half)) = a;            // V = the bank rows themselves: inv_temp is applied once, in qn_fold_k
        *(f32x4*)(myv + banksm::vt_off<D>(c, 16 * s + 8 * half + 4)) = b;
      }
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        bf16x8 kf[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) kf[q] = frag(s, t, q);
        splitbf::mma6_32(acc[t], xb, kf);                               // A: the bank rows (accumulator rows), B: the queries (one per lane)
      }
    }
    [[maybe_unused]] float ipj[16];                                     // Segments: inv_phi of the 16 bank rows this lane holds scores of
    if constexpr (SRC::PER_ROW) {
#pragma unroll
      for (int r = 0; r < 16; ++r) ipj[r] = __shfl(ipr, splitbf::acc32_row(r, half), 64);
    }
    bf16x8 pb[KT][2][3];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      float sc[16], tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = r0 + splitbf::acc32_row(r, half);
        // the score: the product in the call's arithmetic, then ONE fp32 multiply (never contracted into the subtraction below)
        if constexpr (SRC::PER_ROW) {
          const float v = banksm::mul_rn(acc[t][r], ipj[r]);
          if (j == (int64_t)labg[t] && tb + t < T) src.spos[(int64_t)src.seg * mpad + 32 * tt[t] + c] = v;
          sc[r] = j < end ? v : -INFINITY;
        } else {
          sc[r] = j < end ? banksm::mul_rn(acc[t][r], src.inv_temp) : -INFINITY;
        }
        tm = fmaxf(tm, sc[r]);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));                           // both halves of a query rescale the accumulators they share by the same factor
      const float mn = fmaxf(mrun[t], tm);                              // finite from the first tile on: its first row is inside the range
      const float scale = __builtin_amdgcn_exp2f((mrun[t] - mn) * banksm::LOG2E);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {                                    // the exponent from the UNROUNDED product (an fma): the rounding of a score at |s| ~ 20 would cost p 1e-6
        if constexpr (SRC::PER_ROW) sc[r] = sc[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(fmaf(acc[t][r], ipj[r], -mn) * banksm::LOG2E);
        else sc[r] = sc[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(fmaf(acc[t][r], src.inv_temp, -mn) * banksm::LOG2E);
        ps += sc[r];
      }
      lrun[t] = lrun[t] * scale + ps;
      mrun[t] = mn;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[t][dt][r] *= scale;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        splitbf::split8(f32x4{sc[8 * u], sc[8 * u + 1], sc[8 * u + 2], sc[8 * u + 3]}, f32x4{sc[8 * u + 4], sc[8 * u + 5], sc[8 * u + 6], sc[8 * u + 7]}, pb[t][u]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                                    // the tile of V is complete before any lane reads a column of it
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = myv[banksm::vt_off<D>((i & 3) + 16 * u + 8 * (i >> 2) + 4 * half, 32 * dt + c)];   // P's own order: no shuffle on the B side
        bf16x8 va[3];
        splitbf::split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, va);
#pragma unroll
        for (int t = 0; t < KT; ++t) splitbf::mma6_32(out[t][dt], va, pb[t][u]);   // A: 32 columns of V, B: P of the queries
      }
  }
  const int64_t part = (int64_t)sl * 4 + wave;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const float lt = lrun[t] + __shfl_xor(lrun[t], 32, 64);
    if (tb + t >= T) continue;
    const int64_t o = part * mpad + 32 * (tb + t) + c;
    if (half == 0) { pm[o] = mrun[t]; pl[o] = lt; }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(f32x4*)(pacc + o * D + 32 * dt + 8 * g + 4 * half) = f32x4{out[t][dt][4 * g], out[t][dt][4 * g + 1], out[t][dt][4 * g + 2], out[t][dt][4 * g + 3]};
  }
