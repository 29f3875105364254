// Stand-alone driver of csrc/lars_plan.h for a host sanitizer build (tests/test_lars_cpu.py compiles it with -fsanitize=address,undefined and runs it).
// Input (argv[1]): one plan per line - "T expect off_0 .. off_{T-1} numel_0 .. numel_{T-1} flag_0 .. flag_{T-1}", expect = the ssv_status the builder must
// return when given a buffer of exactly the size the sizing helper names ("short" instead of a number: one byte less, which must be refused as too small).
// Every accepted plan is built into a heap buffer of EXACTLY that size (so that a write behind it is an ASan report) and re-checked here: chunks tile every
// tensor once, in order, none longer than LARS_CHUNK_FLOATS, none across a tensor; the tensor table's ranges are contiguous and ascending.  Exit 0 = all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../self-supervised-vision_amd/csrc/lars_plan.h"

static int check_plan(int32_t T, const std::vector<int64_t>& off, const std::vector<int64_t>& num, const std::vector<int32_t>& flag, const void* plan, int64_t chunks) {
  const LarsChunk* ct = (const LarsChunk*)plan;
  const LarsTensor* tt = (const LarsTensor*)((const char*)plan + (size_t)chunks * sizeof(LarsChunk));
  int32_t c = 0;
  for (int32_t t = 0; t < T; ++t) {
    if (tt[t].first != c || tt[t].count < 1) return 1;
    if (tt[t].flags != ((flag[t] ? LARS_DECAY : 0) | (flag[t] ? LARS_ADAPT : 0))) return 2;
    int64_t at = off[t];
    for (int32_t k = 0; k < tt[t].count; ++k, ++c) {
      if (c >= chunks || ct[c].tensor != t || ct[c].start != at || ct[c].len < 1 || ct[c].len > LARS_CHUNK_FLOATS) return 3;
      if (k + 1 < tt[t].count && ct[c].len != LARS_CHUNK_FLOATS) return 4;
      at += ct[c].len;
    }
    if (at != off[t] + num[t]) return 5;
  }
  return c == chunks ? 0 : 6;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s plans.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  int lineno = 0, built = 0, refused = 0;
  char err[256];
  while (std::getline(in, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream ss(line);
    long long T;
    std::string expect;
    ss >> T >> expect;
    const long long Tn = T > 0 ? T : 0;
    std::vector<int64_t> off(Tn), num(Tn);
    std::vector<int32_t> flag(Tn);
    for (auto& v : off) { long long x; ss >> x; v = x; }
    for (auto& v : num) { long long x; ss >> x; v = x; }
    for (auto& v : flag) { long long x; ss >> x; v = (int32_t)x; }
    if (!ss) { fprintf(stderr, "line %d: malformed\n", lineno); return 2; }
    const bool is_short = expect == "short";
    const int want = is_short ? (int)SSV_ERR_WORKSPACE : atoi(expect.c_str());
    const size_t bytes = lars_plan_bytes((int32_t)T, num.data());
    const int64_t chunks = lars_plan_chunks((int32_t)T, num.data());
    const size_t give = is_short && bytes ? bytes - 1 : bytes;
    void* plan = malloc(give ? give : 1);
    memset(plan, 0xA5, give ? give : 1);
    err[0] = 0;
    const int rc = lars_plan_build((int32_t)T, off.data(), num.data(), flag.data(), flag.data(), plan, give, err, sizeof(err));
    int bad = rc != want;
    if (!bad && rc == SSV_OK) { bad = check_plan((int32_t)T, off, num, flag, plan, chunks); ++built; }
    if (!bad && rc != SSV_OK) { bad = err[0] == 0; ++refused; }                    // a refusal says why
    free(plan);
    if (bad) { fprintf(stderr, "line %d: rc %d (expected %d), check %d, message '%s'\n", lineno, rc, want, bad, err); return 1; }
  }
  // NULL tables and a NULL buffer are refused, not followed
  int64_t one = 1, zero = 0;
  int32_t f = 1;
  char buf[64];
  if (lars_plan_build(1, nullptr, &one, &f, &f, buf, sizeof(buf), err, sizeof(err)) != SSV_ERR_INVALID) return 1;
  if (lars_plan_build(1, &zero, &one, &f, &f, nullptr, 64, err, sizeof(err)) != SSV_ERR_INVALID) return 1;
  if (lars_plan_build(1, &zero, &one, &f, &f, buf, sizeof(buf), nullptr, 0) != SSV_OK) return 1;
  if (lars_plan_bytes(0, &one) != 0 || lars_plan_chunks(1, nullptr) != 0) return 1;
  printf("lars plans: %d built and checked, %d refused\n", built, refused);
  return 0;
}
