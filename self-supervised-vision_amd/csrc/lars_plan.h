// The LARS plan (csrc/lars.hip): how the flat parameter arena is cut into the chunks the two LARS kernels work on, one workgroup per chunk.  Plain C++, no device
// code and no HIP header, so that a host-only program can compile it on its own (tests/lars_plan_main.cpp does, under ASan + UBSan).
//
// plan = [chunk table: nchunks x LarsChunk][tensor table: T x LarsTensor], 16 bytes per record, built once per optimizer on the host and uploaded as it is.
//   * a chunk is at most LARS_CHUNK_FLOATS floats of ONE tensor: tensor t of numel m becomes ceil(m / LARS_CHUNK_FLOATS) chunks, all full but the last;
//   * chunks are numbered tensor by tensor, so a tensor's chunks are the contiguous range [first, first + count) - the order its partial norms are folded in;
//   * the padding floats between tensors (utils/train_utils.ParamArena aligns every tensor to 64 floats) belong to no chunk: never read into a norm, never written;
//   * tensor offsets are multiples of 4 floats and so is LARS_CHUNK_FLOATS: every chunk starts on a float4 of a 16-byte-aligned arena.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/ssv_hip.h"

constexpr int32_t LARS_CHUNK_FLOATS = 8192;          // 32 floats per thread of a 256-thread workgroup; a 2.4 M-element filter folds 288 partials
constexpr int64_t LARS_MAX_ARENA = (int64_t)1 << 40; // floats; keeps every sum below in int64 and the chunk count in int32
enum : int32_t { LARS_DECAY = 1, LARS_ADAPT = 2 };

struct LarsChunk { int64_t start; int32_t len; int32_t tensor; };
struct LarsTensor { int32_t first; int32_t count; int32_t flags; int32_t reserved; };
static_assert(sizeof(LarsChunk) == 16 && sizeof(LarsTensor) == 16, "the plan's records are 16 bytes: the kernels read them as they are");

// chunks of T tensors of the given sizes; 0 = refused (T < 1, a NULL table, numel < 1, more than LARS_MAX_ARENA floats or 2^31 - 1 chunks)
inline int64_t lars_plan_chunks(int32_t T, const int64_t* numel) {
  if (T < 1 || !numel) return 0;
  int64_t chunks = 0, total = 0;
  for (int32_t t = 0; t < T; ++t) {
    if (numel[t] < 1 || numel[t] > LARS_MAX_ARENA) return 0;
    total += numel[t];
    if (total > LARS_MAX_ARENA) return 0;
    chunks += (numel[t] + LARS_CHUNK_FLOATS - 1) / LARS_CHUNK_FLOATS;
  }
  return chunks <= INT32_MAX ? chunks : 0;
}

inline size_t lars_plan_bytes(int32_t T, const int64_t* numel) {
  const int64_t chunks = lars_plan_chunks(T, numel);
  return chunks ? (size_t)chunks * sizeof(LarsChunk) + (size_t)T * sizeof(LarsTensor) : 0;
}

// Builds the plan into `plan` (a HOST buffer of plan_bytes).  offset[t], numel[t]: tensor t's place in the arena, in floats; decay[t], adapt[t] != 0: the
// tensor is weight-decayed / its step is scaled by the trust ratio.  Returns an ssv_status; a refusal leaves its reason in err (errlen bytes) and `plan` untouched.
inline int lars_plan_build(int32_t T, const int64_t* offset, const int64_t* numel, const int32_t* decay, const int32_t* adapt,
                           void* plan, size_t plan_bytes, char* err, size_t errlen) {
#define LARS_PLAN_REFUSE(code, ...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return (code); } while (0)
  if (T < 1) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: T >= 1 (got %d)", T);
  if (!offset || !numel || !decay || !adapt || !plan) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: null pointer");
  int64_t end = 0;                                                                      // one past the previous tensor
  for (int32_t t = 0; t < T; ++t) {
    if (numel[t] < 1 || numel[t] > LARS_MAX_ARENA) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: tensor %d has numel %lld (need 1 .. 2^40)", t, (long long)numel[t]);
    if (offset[t] < 0 || offset[t] > LARS_MAX_ARENA) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: tensor %d has offset %lld (need 0 .. 2^40)", t, (long long)offset[t]);
    if (offset[t] & 3) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: tensor %d starts at float %lld, not a multiple of 4", t, (long long)offset[t]);
    if (t > 0 && offset[t] <= offset[t - 1]) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: offsets must ascend (tensor %d at %lld after %lld)", t, (long long)offset[t], (long long)offset[t - 1]);
    if (offset[t] < end) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: tensor %d at %lld overlaps tensor %d, which ends at %lld", t, (long long)offset[t], t - 1, (long long)end);
    end = offset[t] + numel[t];
    if (end > LARS_MAX_ARENA) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: tensor %d ends at float %lld (> 2^40)", t, (long long)end);
  }
  const int64_t chunks = lars_plan_chunks(T, numel);
  if (!chunks) LARS_PLAN_REFUSE(SSV_ERR_INVALID, "lars plan: more than 2^31 - 1 chunks");
  const size_t need = (size_t)chunks * sizeof(LarsChunk) + (size_t)T * sizeof(LarsTensor);
  if (plan_bytes < need) LARS_PLAN_REFUSE(SSV_ERR_WORKSPACE, "lars plan: buffer %zu < %zu bytes", plan_bytes, need);
#undef LARS_PLAN_REFUSE
  LarsChunk* ct = (LarsChunk*)plan;
  LarsTensor* tt = (LarsTensor*)((char*)plan + (size_t)chunks * sizeof(LarsChunk));
  int32_t c = 0;
  for (int32_t t = 0; t < T; ++t) {
    const int32_t count = (int32_t)((numel[t] + LARS_CHUNK_FLOATS - 1) / LARS_CHUNK_FLOATS);
    tt[t] = LarsTensor{c, count, (decay[t] ? LARS_DECAY : 0) | (adapt[t] ? LARS_ADAPT : 0), 0};
    for (int32_t k = 0; k < count; ++k, ++c) {
      const int64_t done = (int64_t)k * LARS_CHUNK_FLOATS, left = numel[t] - done;
      ct[c] = LarsChunk{offset[t] + done, (int32_t)(left < LARS_CHUNK_FLOATS ? left : LARS_CHUNK_FLOATS), t};
    }
  }
  return SSV_OK;
}
