// Stand-alone host check of the argument handling of the impnn_pareto_* entries: every call below fails a rule or has
// zero work, so it returns before a launch and no pointer is dereferenced.  Build it together with the library's
// sources with the host-side sanitizers and run it where no GPU is needed:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         ionic_mpnn_amd/csrc/*.hip tools/pareto_args_check.cpp -o pareto_args_check && ./pareto_args_check
#include <cstdio>
#include <cstring>

#include "../include/impnn.h"

namespace {
struct Args {
  const float *f1, *f2;
  const uint32_t* where = nullptr;
  int largest1 = 0, largest2 = 1, restart = 0;
  int64_t row0 = 0, capacity = 64;
  float* values;
  int32_t *cation, *anion;
  void* ws;
  size_t ws_bytes = (size_t)1 << 40;
  int rows = 3, A = 4;
  Args() {
    float* p = reinterpret_cast<float*>(0x100000);  // a stand-in pointer, never dereferenced
    f1 = f2 = p, values = p, cation = anion = reinterpret_cast<int32_t*>(p), ws = p;
  }
};
// entries 0 .. 2 take a row-block, 3 and 4 the workspace alone
int call(int entry, const Args& a) {
  switch (entry) {
    case 0: return impnn_pareto_range(a.f1, a.f2, a.where, a.largest1, a.largest2, a.ws, a.ws_bytes, a.rows, a.A, nullptr);
    case 1: return impnn_pareto_minima(a.f1, a.f2, a.where, a.largest1, a.largest2, a.ws, a.ws_bytes, a.rows, a.A, nullptr);
    case 2: return impnn_pareto_collect(a.f1, a.f2, a.where, a.largest1, a.largest2, a.row0, a.restart, a.values, a.cation,
                                        a.anion, a.capacity, a.ws, a.ws_bytes, a.rows, a.A, nullptr);
    case 3: return impnn_pareto_begin(a.ws, a.ws_bytes, nullptr);
    default: return impnn_pareto_staircase(a.ws, a.ws_bytes, nullptr);
  }
}
int failures = 0;
void expect(const char* what, int entry, int got, int want) {
  if (got != want) ++failures, std::printf("FAIL entry %d %s: %d, expected %d (%s)\n", entry, what, got, want, impnn_last_error_string());
}
template <class T>
T* at(uintptr_t address) { return reinterpret_cast<T*>(address); }
}  // namespace

int main() {
  size_t need = 0;
  if (impnn_pareto_workspace_bytes(&need) != IMPNN_OK || need != 32 + 2 * 4 * ((size_t)1 << impnn_pareto_bucket_bits())) ++failures;
  if (impnn_pareto_workspace_bytes(nullptr) != IMPNN_E_BADARG || impnn_pareto_bucket_bits() != 14) ++failures;
  if (sizeof(impnn_pareto_header) != 32) ++failures;
  for (int e = 0; e < 5; ++e) {
    // (bad argument, code): the table of tests/test_pareto_host.py
#define BAD(code, stmt)                 \
  do {                                  \
    Args a;                             \
    stmt;                               \
    expect(#stmt, e, call(e, a), code); \
  } while (0)
    BAD(IMPNN_E_BADARG, a.ws = nullptr);
    BAD(IMPNN_E_BADARG, a.ws = at<void>(0x100004));
    BAD(IMPNN_E_WORKSPACE, a.ws_bytes = 8);
    BAD(IMPNN_E_WORKSPACE, a.ws_bytes = need - 1);
    if (e >= 3) continue;
    BAD(IMPNN_E_BADARG, a.rows = -1);
    BAD(IMPNN_E_BADARG, a.A = -1);
    BAD(IMPNN_E_BADARG, a.largest1 = 2);
    BAD(IMPNN_E_BADARG, a.largest2 = -1);
    BAD(IMPNN_E_BADARG, (a.rows = -1, a.f1 = nullptr));
    BAD(IMPNN_OK, (a.rows = 0, a.f1 = a.f2 = nullptr, a.ws = nullptr, a.ws_bytes = 0));
    BAD(IMPNN_OK, (a.A = 0, a.values = nullptr, a.cation = a.anion = nullptr));
    BAD(IMPNN_E_BADARG, a.f1 = nullptr);
    BAD(IMPNN_E_BADARG, a.f2 = nullptr);
    BAD(IMPNN_E_BADARG, a.f1 = at<const float>(0x100002));
    BAD(IMPNN_E_BADARG, a.f2 = at<const float>(0x100001));
    BAD(IMPNN_E_BADARG, a.where = at<const uint32_t>(0x100002));
    BAD(IMPNN_E_UNSUPPORTED, (a.rows = 1 << 16, a.A = 1 << 15));
    BAD(IMPNN_E_WORKSPACE, (a.rows = 1 << 16, a.A = 1 << 15, a.ws_bytes = 8));  // the size before the limits
    if (e == 2) {
      BAD(IMPNN_E_BADARG, a.row0 = -1);
      BAD(IMPNN_E_BADARG, a.capacity = -1);
      BAD(IMPNN_E_BADARG, a.values = nullptr);
      BAD(IMPNN_E_BADARG, a.cation = nullptr);
      BAD(IMPNN_E_BADARG, a.anion = nullptr);
      BAD(IMPNN_E_BADARG, a.values = at<float>(0x100002));
      BAD(IMPNN_E_BADARG, a.anion = at<int32_t>(0x100003));
      BAD(IMPNN_E_UNSUPPORTED, a.row0 = ((int64_t)1 << 31) - 3);
      BAD(IMPNN_E_UNSUPPORTED, (a.capacity = 0, a.values = nullptr, a.cation = a.anion = nullptr, a.row0 = ((int64_t)1 << 31) - 3));
    }
#undef BAD
  }
  std::printf(failures ? "%d failures\n" : "pareto_args_check: ok\n", failures);
  return failures != 0;
}
