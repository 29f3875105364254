// Stand-alone driver of csrc/bn_plan.h for a host sanitizer build (tests/test_gpu_bn_pool_kernels.py compiles it with -fsanitize=address,undefined and runs it).
// Input (argv[1]): one query per line - "plan M C", "merge groups cap" or "pool H W".  Output, one line per query:
//   plan M C -> C4 CT RT GY rpb nblk | apply rpb nblk | workspace floats
//   merge groups cap -> factor ncoarse     (factor 0: the one-level merge)
//   pool H W -> Ho Wo
// The workspace of every plan is carved both ways into a heap buffer of EXACTLY the floats the plan names and its ends are touched, so a layout that runs
// past the size is an ASan report.  Exit 0 = every line answered.
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <sstream>
#include <string>
#include "../self-supervised-vision_amd/csrc/bn_plan.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s queries.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  std::string line;
  int lineno = 0, plans = 0, merges = 0;
  while (std::getline(in, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string what;
    long long a, b;
    ss >> what >> a >> b;
    if (!ss || (what != "plan" && what != "merge" && what != "pool") || a < 1 || b < 0) { fprintf(stderr, "line %d: malformed\n", lineno); return 2; }
    if (what == "merge") {
      const MergePlan m = merge_plan(a, b);
      printf("merge %lld %lld -> %d %d\n", a, b, m.factor, m.ncoarse);
      ++merges;
      continue;
    }
    if (what == "pool") {
      printf("pool %lld %lld -> %d %d\n", a, b, pooled_extent((int)a), pooled_extent((int)b));
      continue;
    }
    const int C = (int)b;
    if (C < 4 || C % 4 || a >= (1ll << 31)) { fprintf(stderr, "line %d: need C %% 4 == 0 and M < 2^31\n", lineno); return 2; }
    const BnPlan p = bn_plan(a, C);
    const ApplyGrid g = apply_grid(p, a);
    const size_t floats = bn_ws_floats(p, C);
    float* ws = (float*)malloc(floats * sizeof(float));
    if (!ws) return 2;
    const BnWs pf = ws_partials_first(ws, p, C), vf = ws_vectors_first(ws, C);
    pf.a[0] = pf.b[0] = pf.u[0] = 1.f;
    pf.v[C - 1] = 2.f;                                                            // the last float of the partials-first layout
    vf.u[0] = vf.v[0] = 3.f;
    vf.a[bn_coarse_floats(p, C) - 1] = 4.f;                                       // ... and of the vectors-first one
    const bool ends = pf.v + C == ws + floats && vf.a + bn_coarse_floats(p, C) == ws + floats && ws[floats - 1] == 4.f;
    free(ws);
    if (!ends) { fprintf(stderr, "line %d: a layout does not end where the workspace ends\n", lineno); return 1; }
    printf("plan %lld %d -> %d %d %d %d %d %d | %d %d | %zu\n", a, C, p.C4, p.CT, p.RT, p.GY, p.rpb, p.nblk, g.rpb, g.nblk, floats);
    ++plans;
  }
  printf("bn plans: %d plans, %d merges\n", plans, merges);
  return 0;
}
