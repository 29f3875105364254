// PIRL (models/pirl.py, utils/losses.py:92-117): the per-sample memory bank lives in HBM and the loss reads it BY INDEX.
//   PirlLoss      utils/losses.py:92-117   two cross-entropies over [positive | K negatives] that share the negatives' log-sum-exp
//   MemoryBank    models/pirl.py:33-39     momentum update of the batch's rows (initialize_vectors is the m = 0 case on a zero bank)
//   EncoderModel  models/pirl.py:66-71     the jigsaw cut of an image batch into patches, x-major then y
//
// The negative logits n_ik = bank[pos[i]] . bank[neg[k]] / T are products of bank rows with bank rows: they carry no gradient and both cross-entropies see the
// same L_i = logsumexp_k n_ik.  So the B x K logit matrix never exists in HBM: pirl_lse_k forms it 32 x 32 at a time on v_mfma_f32_32x32x2_f32 (exact fp32, the
// arithmetic of the NT-Xent kernels in loss.hip) with BOTH operands gathered by index - the 32 positive rows of a row block into LDS once, the negatives' rows
// straight from the bank into the A fragments - and keeps a running (max, sum) per row.  K is cut into splits (grid.y) when B alone leaves the device empty; every
// split leaves its (max, sum) in the workspace and pirl_rows_k folds them in split order, so two runs are bit-identical.  pirl_rows_k then owns one row per
// wavefront: the two positive logits, the row's loss term (a double partial, summed by pirl_loss_sum_k) and the gradient - a per-row scalar times bank[pos[i]],
// pushed through the L2 normalisation like ssv_l2norm_bwd does.
#include "common.h"
#include <algorithm>

namespace {

// floats per staged row: +4 keeps the 16-byte reads of 32 rows off one LDS bank group; the widest rows go without so that 32 of them stay within 64 KiB
__host__ __device__ __forceinline__ int lse_lda(int D) { const int w = 8 * ((D + 7) / 8); return w < 512 ? w + 4 : w; }
__device__ __forceinline__ int crow32(int j, int h) { return (j & 3) + 8 * (j >> 2) + 4 * h; }     // row of accumulator register j in a 32x32 MFMA result

// grid (row blocks of 32, K splits), 256 threads.  part[split][row] = (running max, running sum) of the row's negative logits over this split's tiles.
// An index outside [0, N) is never dereferenced: a bad positive makes its row zero, a bad negative is masked out of the sum, and *flag is raised.
__global__ void __launch_bounds__(256)
pirl_lse_k(int N, int D, int B, int K, const float* __restrict__ bank, const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, float inv_temp,
           int tiles_per_split, float* __restrict__ part, int* __restrict__ flag) {
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int DQ = (D + 7) >> 3, lda = lse_lda(D);                      // row stride of the staged positives: whole 8-wide steps, zero filled
  float* smA = sm;                                                     // [32][lda]
  float* sm_m = sm;                                                    // [4][32], [4][32]: the wavefronts' results, over smA once the sweep is done
  float* sm_s = sm + 128;
  const int row0 = blockIdx.x * 32;
  bool bad = false;
  {
    const int q4 = lda >> 2;
    for (int e = tid; e < 32 * q4; e += 256) {
      const int r = e / q4, c = (e - r * q4) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row0 + r < B && c < D) {
        const int64_t p = pos[row0 + r];
        if (p >= 0 && p < N) v = *reinterpret_cast<const f32x4*>(bank + (size_t)p * D + c);
        else bad = true;
      }
      *reinterpret_cast<f32x4*>(smA + r * lda + c) = v;
    }
  }
  __syncthreads();

  float m = -INFINITY, s = 0.f;
  const int ntile = (K + 31) >> 5;
  const int t0 = blockIdx.y * tiles_per_split, t1 = min(ntile, t0 + tiles_per_split);
  const float* arow = smA + l31 * lda + 4 * h;
  for (int ct = t0 + wave; ct < t1; ct += 4) {
    const int cl = ct * 32 + l31;
    int64_t nidx = cl < K ? neg[cl] : 0;
    const bool nvalid = cl < K && nidx >= 0 && nidx < N;
    if (cl < K && !nvalid) bad = true;
    if (!nvalid) nidx = 0;                                             // row 0 exists (N >= 1); its products are masked below
    const unsigned long long ok = __ballot(nvalid);                    // bit c (c < 32): column ct * 32 + c takes part
    const float* brow = bank + (size_t)nidx * D + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int q = 0; q < DQ; ++q) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (8 * q + 4 * h < D) a = *reinterpret_cast<const f32x4*>(brow + 8 * q);
      const f32x4 b = *reinterpret_cast<const f32x4*>(arow + 8 * q);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[t], acc, 0, 0, 0);
    }
    // acc[j]: negative crow32(j, h) of this tile against block row l31
    float sv[16];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      sv[j] = ((ok >> crow32(j, h)) & 1ull) ? acc[j] * inv_temp : -INFINITY;
      tmax = fmaxf(tmax, sv[j]);
    }
    if (tmax > -INFINITY) {
      const float mn = fmaxf(m, tmax);
      float add = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) add += expf(sv[j] - mn);            // exp(-inf) = 0 for masked entries
      s = s * expf(m - mn) + add;
      m = mn;
    }
  }
  {   // the two half-waves hold the same row, disjoint negatives
    const float m2 = __shfl_xor(m, 32, 64), s2 = __shfl_xor(s, 32, 64);
    const float mn = fmaxf(m, m2);
    s = (m > -INFINITY ? s * expf(m - mn) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mn) : 0.f);
    m = mn;
  }
  __syncthreads();                                                     // every wavefront has left smA
  if (h == 0) { sm_m[wave * 32 + l31] = m; sm_s[wave * 32 + l31] = s; }
  __syncthreads();
  if (wave == 0 && h == 0 && row0 + l31 < B) {
    float mm = sm_m[l31], ss = sm_s[l31];
    for (int w = 1; w < 4; ++w) {
      const float m2 = sm_m[w * 32 + l31], s2 = sm_s[w * 32 + l31];
      const float mn = fmaxf(mm, m2);
      ss = (mm > -INFINITY ? ss * expf(mm - mn) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mn) : 0.f);
      mm = mn;
    }
    float* p = part + ((size_t)blockIdx.y * B + row0 + l31) * 2;
    p[0] = mm; p[1] = ss;
  }
  if (bad) atomicOr(flag, 1);
}

// one wavefront per row: L_i from the splits (in split order), the two positive logits, the row's loss term and both gradients
//   loss_i = w (lse(p1, L) - p1) + (1 - w) (lse(p2, L) - p2),   p1 = m . v_patch / T,   p2 = m . v_img / T,   v = z / max(|z|, eps) when normalising
//   d loss / d v = g m with g = weight (sigma - 1) / (B T), sigma = exp(p - lse(p, L));   d z = (d v - v (v . d v)) / max(|z|, eps)
__global__ void __launch_bounds__(256)
pirl_rows_k(int N, int D, int B, int splits, const float* __restrict__ bank, const int64_t* __restrict__ pos, const float* __restrict__ zimg,
            const float* __restrict__ zpatch, int normalize, float eps, float inv_temp, float w, const float* __restrict__ part,
            float* __restrict__ dimg, float* __restrict__ dpatch, double* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  float L = -INFINITY;
  {
    float mm = -INFINITY, ss = 0.f;
    for (int sp = 0; sp < splits; ++sp) {
      const float m2 = part[((size_t)sp * B + r) * 2], s2 = part[((size_t)sp * B + r) * 2 + 1];
      const float mn = fmaxf(mm, m2);
      ss = (mm > -INFINITY ? ss * expf(mm - mn) : 0.f) + (m2 > -INFINITY ? s2 * expf(m2 - mn) : 0.f);
      mm = mn;
    }
    if (mm > -INFINITY) L = mm + logf(ss);
  }
  const int64_t p = pos[r];
  const bool pvalid = p >= 0 && p < N;                                 // pirl_lse_k has raised the flag otherwise
  const float* mrow = bank + (size_t)(pvalid ? p : 0) * D;
  const float* zi = zimg + (size_t)r * D;
  const float* zp = zpatch + (size_t)r * D;
  float si = 0.f, sp2 = 0.f, di = 0.f, dp = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float mv = pvalid ? mrow[d] : 0.f, a = zi[d], b = zp[d];
    si += a * a; sp2 += b * b; di += mv * a; dp += mv * b;
  }
  si = wave_sum(si); sp2 = wave_sum(sp2); di = wave_sum(di); dp = wave_sum(dp);
  const float inv_i = normalize ? 1.f / fmaxf(sqrtf(si), eps) : 1.f, inv_p = normalize ? 1.f / fmaxf(sqrtf(sp2), eps) : 1.f;
  const float mvi = di * inv_i, mvp = dp * inv_p;                      // m . v
  const float p1 = mvp * inv_temp, p2 = mvi * inv_temp;
  auto lse2 = [](float a, float b) { const float mx = fmaxf(a, b); return mx + logf(expf(a - mx) + expf(b - mx)); };
  const float l1 = lse2(p1, L), l2 = lse2(p2, L);
  const float g1 = w * (expf(p1 - l1) - 1.f) * inv_temp / (float)B, g2 = (1.f - w) * (expf(p2 - l2) - 1.f) * inv_temp / (float)B;
  for (int d = lane; d < D; d += 64) {
    const float mv = pvalid ? mrow[d] : 0.f;
    if (normalize) {
      dpatch[(size_t)r * D + d] = g1 * (mv - zp[d] * inv_p * mvp) * inv_p;
      dimg[(size_t)r * D + d] = g2 * (mv - zi[d] * inv_i * mvi) * inv_i;
    } else {
      dpatch[(size_t)r * D + d] = g1 * mv;
      dimg[(size_t)r * D + d] = g2 * mv;
    }
  }
  if (lane == 0) rowloss[r] = (double)w * (double)(l1 - p1) + (double)(1.f - w) * (double)(l2 - p2);
}

__global__ void pirl_loss_sum_k(int B, const double* __restrict__ rowloss, float* __restrict__ loss) {
  __shared__ double sm[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 256) s += rowloss[i];
  sm[threadIdx.x] = s;
  __syncthreads();
  SSV_BLOCK_SUM_256(sm);
  if (threadIdx.x == 0) *loss = (float)(sm[0] / (double)B);
}

// bank[idx[i]] = m bank[idx[i]] + (1 - m) z_i / max(|z_i|, eps): one wavefront per batch row; an index outside [0, N) is skipped
__global__ void __launch_bounds__(256)
bank_momentum_k(int N, int D, int n, float* __restrict__ bank, const int64_t* __restrict__ idx, const float* __restrict__ z, float m, float eps) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t row = idx[i];
  if (row < 0 || row >= N) return;
  const float* src = z + (size_t)i * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += src[d] * src[d];
  const float nrm = fmaxf(sqrtf(wave_sum(s)), eps), keep = 1.f - m;
  float* dst = bank + (size_t)row * D;
  for (int d = lane; d < D; d += 64) dst[d] = m * dst[d] + keep * (src[d] / nrm);
}

// x [B][H][W][C] -> out [P][B][ps][ps][C], patch p = xi * (H / ps) + yi covering rows yi*ps.., columns xi*ps.. (models/pirl.py:67-71 loops x outside y)
__global__ void __launch_bounds__(256)
patch_split_k(int64_t total, int B, int H, int W, int C, int ps, const float* __restrict__ x, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ny = H / ps;
  int64_t t = e;
  const int c = (int)(t % C); t /= C;
  const int px = (int)(t % ps); t /= ps;
  const int py = (int)(t % ps); t /= ps;
  const int b = (int)(t % B); t /= B;
  const int p = (int)t, xi = p / ny, yi = p - xi * ny;
  out[e] = x[(((int64_t)b * H + (yi * ps + py)) * W + (xi * ps + px)) * C + c];
}

int lse_tiles(int K) { return (K + 31) / 32; }
int lse_lds_bytes(int D) { return 32 * lse_lda(D) * (int)sizeof(float); }

}  // namespace

// K splits at this shape: enough workgroups for two per compute unit where the negatives allow, every split at least one tile per wavefront
extern "C" int64_t ssv_pirl_default_splits(int32_t B, int32_t K) {
  if (B <= 0 || K <= 0) return 1;
  const int splits = std::min(512 / std::max(cdiv(B, 32), 1), lse_tiles(K) / 4);
  return std::max(1, std::min(splits, 64));
}

// flag word (256 bytes kept for alignment) | (max, sum) partials [splits][B][2] | double row terms [B]
extern "C" size_t ssv_pirl_loss_workspace_bytes(int32_t B, int32_t splits) {
  if (B <= 0 || splits <= 0) return 0;
  return 256 + ((size_t)splits * B * 2 * sizeof(float) + 255) / 256 * 256 + (size_t)B * sizeof(double);
}

extern "C" int ssv_pirl_loss_fwd_bwd(int64_t N, int32_t D, int32_t B, int32_t K, const float* bank, const void* pos_index, const void* neg_index,
                                     const float* img_features, const float* patch_features, int32_t normalize, float inv_temp, float loss_weight,
                                     int32_t splits, float* loss, float* d_img, float* d_patch, void* ws, size_t ws_bytes, void* stream) {
  SSV_REQUIRE(N > 0 && N < ((int64_t)1 << 31) && D > 0 && B > 0 && K > 0 && bank && pos_index && neg_index && img_features && patch_features && loss && d_img &&
              d_patch && ws, "ssv_pirl_loss_fwd_bwd: bad arguments");
  SSV_REQUIRE(D % 4 == 0 && D <= 512, "ssv_pirl_loss_fwd_bwd: D must be a multiple of 4, at most 512 (got %d)", D);
  SSV_REQUIRE(((uintptr_t)bank & 15) == 0 && ((uintptr_t)ws & 255) == 0, "ssv_pirl_loss_fwd_bwd: bank must be 16-byte aligned, the workspace 256-byte aligned");
  SSV_REQUIRE(splits >= 0, "ssv_pirl_loss_fwd_bwd: splits must be 0 (library default) or positive");
  const int ntile = lse_tiles(K);
  if (splits == 0) splits = (int)ssv_pirl_default_splits(B, K);
  splits = std::max(1, std::min(std::min(splits, ntile), 64));
  const int tiles_per_split = cdiv(ntile, splits);
  splits = cdiv(ntile, tiles_per_split);                               // no empty split
  if (ws_bytes < ssv_pirl_loss_workspace_bytes(B, splits)) SSV_FAIL(SSV_ERR_WORKSPACE, "ssv_pirl_loss_fwd_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_LOSS, s);
  int* flag = (int*)ws;
  float* part = (float*)((char*)ws + 256);
  double* rowloss = (double*)((char*)ws + 256 + ((size_t)splits * B * 2 * sizeof(float) + 255) / 256 * 256);
  if (hipMemsetAsync(flag, 0, 256, s) != hipSuccess) SSV_FAIL(SSV_ERR_LAUNCH, "ssv_pirl_loss_fwd_bwd: could not clear the flag word");
  hipLaunchKernelGGL(pirl_lse_k, dim3(cdiv(B, 32), splits), dim3(256), lse_lds_bytes(D), s, (int)N, D, B, K, bank, (const int64_t*)pos_index,
                     (const int64_t*)neg_index, inv_temp, tiles_per_split, part, flag);
  hipLaunchKernelGGL(pirl_rows_k, dim3(cdiv(B, 4)), dim3(256), 0, s, (int)N, D, B, splits, bank, (const int64_t*)pos_index, img_features, patch_features,
                     normalize, 1e-12f, inv_temp, loss_weight, (const float*)part, d_img, d_patch, rowloss);
  hipLaunchKernelGGL(pirl_loss_sum_k, dim3(1), dim3(256), 0, s, B, (const double*)rowloss, loss);
  SSV_CHECK_LAUNCH("ssv_pirl_loss_fwd_bwd");
  return SSV_OK;
}

extern "C" int ssv_bank_momentum_update(int64_t N, int32_t D, float* bank, int32_t n, const void* index, const float* z, float momentum, float eps, void* stream) {
  SSV_REQUIRE(N > 0 && N < ((int64_t)1 << 31) && D > 0 && n > 0 && bank && index && z, "ssv_bank_momentum_update: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(bank_momentum_k, dim3(cdiv(n, 4)), dim3(256), 0, s, (int)N, D, n, bank, (const int64_t*)index, z, momentum, eps);
  SSV_CHECK_LAUNCH("ssv_bank_momentum_update");
  return SSV_OK;
}

extern "C" int ssv_patch_split(int32_t B, int32_t H, int32_t W, int32_t C, int32_t patch, const float* x, float* out, void* stream) {
  SSV_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && patch > 0 && x && out, "ssv_patch_split: bad arguments");
  SSV_REQUIRE(H % patch == 0 && W % patch == 0, "ssv_patch_split: the patch size %d does not divide %d x %d", patch, H, W);
  const int64_t total = (int64_t)B * H * W * C;
  SSV_REQUIRE(total < ((int64_t)1 << 31) * 256, "ssv_patch_split: batch too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(SSV_PROF_MISC, s);
  hipLaunchKernelGGL(patch_split_k, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, total, B, H, W, C, patch, x, out);
  SSV_CHECK_LAUNCH("ssv_patch_split");
  return SSV_OK;
}
