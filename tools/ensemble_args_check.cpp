// Stand-alone host check of the argument handling of the impnn_ensemble_grid* entries: every call below fails a rule or
// has zero work, so it returns before a launch and no pointer is dereferenced.  Build it together with the library's
// sources with the host-side sanitizers and run it where no GPU is needed:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         ionic_mpnn_amd/csrc/*.hip tools/ensemble_args_check.cpp -o ensemble_args_check && ./ensemble_args_check
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../include/impnn.h"

namespace {
struct Args {
  int kind = 0, M = 3;
  const float *mc, *ma, *T, *tails;
  float kappa = 1.0f, lo = 0.f, hi = 1.f;
  float *mean, *std, *score, *values;
  uint32_t* words;
  const uint32_t* where;
  int32_t *cation, *anion;
  void* ws;
  size_t ws_bytes = (size_t)1 << 40;
  int k = 5, C = 3, A = 4, nT = 2, F = 32, Mx = 20, workgroups = 0;
  Args() {
    float* p = reinterpret_cast<float*>(0x100000);  // a stand-in pointer, never dereferenced
    mc = ma = T = tails = p, mean = std = score = values = p;
    words = reinterpret_cast<uint32_t*>(p), where = words, cation = anion = reinterpret_cast<int32_t*>(p), ws = p;
  }
};
int call(int entry, const Args& a) {
  switch (entry) {
    case 0: return impnn_ensemble_grid(a.kind, a.M, a.mc, a.ma, a.T, a.tails, a.kappa, a.mean, a.std, a.score, a.C, a.A, a.nT, a.F, a.Mx, nullptr);
    case 1: return impnn_ensemble_grid_mask(a.kind, a.M, a.mc, a.ma, a.T, a.tails, a.kappa, a.lo, a.hi, a.words, a.C, a.A, a.nT, a.F, a.Mx, nullptr);
    case 2: return impnn_ensemble_grid_topk(a.kind, a.M, a.mc, a.ma, a.T, a.tails, a.kappa, a.k, 0, a.values, a.cation, a.anion, a.ws, a.ws_bytes, a.C, a.A, a.nT, a.F, a.Mx, a.workgroups, nullptr);
    default: return impnn_ensemble_grid_topk_where(a.kind, a.M, a.mc, a.ma, a.T, a.tails, a.kappa, a.where, a.k, 0, a.values, a.cation, a.anion, a.ws, a.ws_bytes, a.C, a.A, a.nT, a.F, a.Mx, a.workgroups, nullptr);
  }
}
int failures = 0;
void expect(const char* what, int entry, int got, int want) {
  if (got != want) ++failures, std::printf("FAIL entry %d %s: %d, expected %d (%s)\n", entry, what, got, want, impnn_last_error_string());
}
}  // namespace

int main() {
  const float nan = std::nanf(""), inf = INFINITY;
  for (int e = 0; e < 4; ++e) {
    // (bad argument, code): the table of tests/test_ensemble_host.py
#define BAD(code, stmt)          \
  do {                           \
    Args a;                      \
    stmt;                        \
    expect(#stmt, e, call(e, a), code); \
  } while (0)
    BAD(IMPNN_E_BADARG, a.kind = 2);
    BAD(IMPNN_E_BADARG, a.kind = -1);
    BAD(IMPNN_E_BADARG, a.C = -1);
    BAD(IMPNN_E_BADARG, a.A = -1);
    BAD(IMPNN_E_BADARG, a.nT = -1);
    BAD(IMPNN_E_BADARG, a.F = 0);
    BAD(IMPNN_E_BADARG, a.Mx = -1);
    BAD(IMPNN_E_BADARG, (a.kind = 1, a.nT = 3));
    BAD(IMPNN_E_BADARG, a.nT = 0);
    BAD(IMPNN_E_BADARG, a.M = 0);
    BAD(IMPNN_E_BADARG, a.M = -2);
    BAD(IMPNN_E_UNSUPPORTED, a.M = 9);
    BAD(IMPNN_E_BADARG, a.kappa = nan);
    BAD(IMPNN_E_BADARG, a.kappa = inf);
    BAD(IMPNN_E_BADARG, a.kappa = -inf);
    BAD(IMPNN_E_UNSUPPORTED, a.F = 65);
    BAD(IMPNN_E_UNSUPPORTED, a.Mx = 65);
    BAD(IMPNN_E_BADARG, a.mc = nullptr);
    BAD(IMPNN_E_BADARG, a.ma = nullptr);
    BAD(IMPNN_E_BADARG, a.T = nullptr);
    BAD(IMPNN_E_BADARG, a.tails = nullptr);
    BAD(IMPNN_E_BADARG, (a.kind = 1, a.nT = 0));  // temperatures given to the melting-point grid
    BAD(IMPNN_OK, (a.C = 0, a.mc = nullptr, a.ws = nullptr, a.ws_bytes = 0));
    BAD(IMPNN_OK, (a.A = 0, a.tails = nullptr, a.mean = a.std = a.score = nullptr, a.words = nullptr));
    if (e == 0) {
      BAD(IMPNN_E_BADARG, a.mean = a.std = a.score = nullptr);
      BAD(IMPNN_E_UNSUPPORTED, a.nT = 4097);
    } else if (e == 1) {
      BAD(IMPNN_E_BADARG, a.words = nullptr);
      BAD(IMPNN_E_BADARG, a.lo = nan);
      BAD(IMPNN_E_BADARG, a.hi = nan);
      BAD(IMPNN_E_BADARG, a.words = reinterpret_cast<uint32_t*>(0x100002));
      BAD(IMPNN_E_UNSUPPORTED, a.nT = 4097);
    } else {
      BAD(IMPNN_E_BADARG, a.k = 0);
      BAD(IMPNN_E_UNSUPPORTED, a.k = 1025);
      BAD(IMPNN_E_UNSUPPORTED, a.nT = 5);
      BAD(IMPNN_E_UNSUPPORTED, (a.M = 8, a.nT = 3));
      BAD(IMPNN_E_UNSUPPORTED, (a.C = 1 << 16, a.A = 1 << 16));
      BAD(IMPNN_E_BADARG, a.workgroups = -1);
      BAD(IMPNN_E_BADARG, a.values = nullptr);
      BAD(IMPNN_E_BADARG, a.ws = nullptr);
      BAD(IMPNN_E_BADARG, a.ws = reinterpret_cast<void*>(0x100004));
      BAD(IMPNN_E_WORKSPACE, a.ws_bytes = 0);
      if (e == 3) {
        BAD(IMPNN_E_BADARG, a.where = nullptr);
        BAD(IMPNN_E_BADARG, a.where = reinterpret_cast<const uint32_t*>(0x100002));
      }
    }
#undef BAD
  }
  size_t need = 0;
  if (impnn_ensemble_grid_topk_workspace_bytes(3, 100, 100, 2, 100, 3, &need) != IMPNN_OK || need != 3 * 2 * 100 * 8) ++failures;
  if (impnn_ensemble_grid_topk_workspace_bytes(0, 1, 1, 1, 1, 0, &need) != IMPNN_E_BADARG) ++failures;
  if (impnn_ensemble_grid_topk_workspace_bytes(8, 1, 1, 3, 1, 0, &need) != IMPNN_E_UNSUPPORTED) ++failures;
  if (impnn_ensemble_grid_topk_workspace_bytes(1, 1, 1, 1, 1, 0, nullptr) != IMPNN_E_BADARG) ++failures;
  if (impnn_ensemble_grid_max_members() != 8 || impnn_ensemble_grid_topk_max_temperatures(8) < 1) ++failures;
  if (impnn_ensemble_grid_max_temperatures(0, 8) != 4096 || impnn_ensemble_grid_tail_floats(0, 32, 20) != 63) ++failures;
  std::printf(failures ? "%d failures\n" : "ensemble_args_check: ok\n", failures);
  return failures != 0;
}
