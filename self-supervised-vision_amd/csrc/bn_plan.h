// The BatchNorm / pooling plan (csrc/bn.hip, csrc/pool.hip): how an [M][C] matrix is cut into workgroups, when the merge of the per-block partials takes two
// levels, where the pieces of the workspace lie, and the pooled extent of MaxPool2d(3, 2, 1).  Plain C++, no device code and no HIP header, so that a host-only
// program can compile it on its own (tests/bn_plan_main.cpp does, under ASan + UBSan; tests/test_gpu_bn_pool_kernels.py holds its Python restatement to it).
#pragma once
#include <stddef.h>
#include <stdint.h>

inline int64_t bn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// float4 groups per row, channel groups / row lanes of a 256-thread block, y-blocks, rows per block, blocks
struct BnPlan { int C4, CT, RT, GY, rpb, nblk; };
inline BnPlan bn_plan(int64_t M, int C) {
  BnPlan p;
  p.C4 = C / 4;
  p.CT = p.C4 < 256 ? p.C4 : 256;
  p.RT = 256 / p.CT;
  p.GY = (int)bn_cdiv(p.C4, p.CT);
  int64_t rpb = bn_cdiv(M, 1024);
  const int64_t min_rows = (int64_t)p.RT * 4;
  if (rpb < min_rows) rpb = min_rows;
  p.rpb = (int)rpb;
  p.nblk = (int)bn_cdiv(M, rpb);
  return p;
}

// Grid of the pure element-wise passes (bn_apply_k, bn_bwd_apply_k): their result does not depend on the partition, so they get a
// grid of their own - about 1024 workgroups in all, each walking a long run of rows (profiles/r02_experiments_step_time.txt).
struct ApplyGrid { int rpb, nblk; };
inline ApplyGrid apply_grid(const BnPlan& p, int64_t M) {
  int64_t blocks = 1024 / p.GY;
  if (blocks < 1) blocks = 1;
  int64_t rpb = bn_cdiv(M, blocks);
  const int64_t min_rows = (int64_t)p.RT * 4;
  if (rpb < min_rows) rpb = min_rows;
  ApplyGrid g;
  g.rpb = (int)rpb;
  g.nblk = (int)bn_cdiv(M, rpb);
  return g;
}

// More than 2048 partials per channel are merged in two levels: `factor` consecutive fine partials -> one coarse one (32 of them, or as many as it takes to fit
// `cap` coarse partials), then the usual finalize over `ncoarse`.  factor == 0: one level.
struct MergePlan { int factor, ncoarse; };
inline MergePlan merge_plan(int64_t groups, int64_t cap) {
  MergePlan m = {0, (int)groups};
  if (groups <= 2048) return m;
  m.factor = (int)(cap > 0 && bn_cdiv(groups, 32) > cap ? bn_cdiv(groups, cap) : 32);
  m.ncoarse = (int)bn_cdiv(groups, m.factor);
  return m;
}

// The workspace of every entry point is 2 * nblk * C + 2 * C floats (ssv_bn_workspace_bytes), laid out one of two ways:
//   partials first  [a: nblk * C][b: nblk * C][u: C][v: C]     the entry points that reduce x themselves: pmean | pm2 | scale | shift,  psg | psgx | k1 | k2
//   vectors first   [u: C][v: C][a: room for 2 * nblk * C]     partials handed over by a producer: scale | shift (k1 | k2), then the coarse partials
inline size_t bn_ws_floats(const BnPlan& p, int C) { return (size_t)2 * p.nblk * C + 2 * (size_t)C; }
inline size_t bn_coarse_floats(const BnPlan& p, int C) { return (size_t)2 * p.nblk * C; }
struct BnWs { float *a, *b, *u, *v; };
inline BnWs ws_partials_first(void* ws, const BnPlan& p, int C) {
  float* a = (float*)ws;
  const size_t n = (size_t)p.nblk * C;
  return {a, a + n, a + 2 * n, a + 2 * n + C};
}
inline BnWs ws_vectors_first(void* ws, int C) { return {(float*)ws + 2 * (size_t)C, nullptr, (float*)ws, (float*)ws + C}; }

// MaxPool2d(kernel 3, stride 2, pad 1): outputs along an axis of n inputs
inline int pooled_extent(int n) { return (n + 2 - 3) / 2 + 1; }
