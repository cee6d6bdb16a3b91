// Stand-alone host check of the argument handling of impnn_encoder_prepared_bytes_gates and
// impnn_encoder_prepare_weights_gates (the typed encoder's step-0 gate table behind the message table): every prepare call
// below fails a rule or has nothing to build, so it returns before a launch and no pointer is dereferenced.  Build it
// together with the library's sources with the host-side sanitizers and run it where no GPU is needed:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         ionic_mpnn_amd/csrc/*.hip tools/prepare_gates_args_check.cpp -o prepare_gates_args_check && ./prepare_gates_args_check
#include <cstdio>
#include <cstring>

#include "../include/impnn.h"

namespace {
template <class T>
T* at(uintptr_t address) { return reinterpret_cast<T*>(address); }
struct Args {
  const float *weights, *bond_table, *atom_table;
  void* prepared;
  int Va = 124, D = 32, K = 8, S = 3, Vb = 72, mode = IMPNN_ENCODER_F32_TYPED;
  size_t bytes = (size_t)1 << 40;
  Args() {
    weights = bond_table = atom_table = at<float>(0x100000);  // stand-in pointers, never dereferenced
    prepared = at<void>(0x200000);
  }
};
int call(const Args& a) {
  return impnn_encoder_prepare_weights_gates(a.weights, a.bond_table, a.atom_table, a.Va, a.D, a.K, a.S, a.Vb, a.mode,
                                             a.prepared, a.bytes, nullptr);
}
int failures = 0;
void expect(const char* what, int got, int want) {
  if (got != want) ++failures, std::printf("FAIL %s: %d, expected %d (%s)\n", what, got, want, impnn_last_error_string());
}
void expect_size(const char* what, size_t got, size_t want) {
  if (got != want) ++failures, std::printf("FAIL %s: %zu, expected %zu\n", what, got, want);
}
}  // namespace

int main() {
  // ---- the size query: the with-atoms size plus (Va + 1) x 256 B where a message table is built, else that size itself
  for (int mode = IMPNN_ENCODER_F32_TYPED; mode <= IMPNN_ENCODER_F32X3_TYPED; ++mode) {
    const size_t old = impnn_encoder_prepared_bytes(32, 3, 72, mode);
    expect_size("bench vocabulary", impnn_encoder_prepared_bytes_gates(32, 3, 124, 72, mode),
                impnn_encoder_prepared_bytes_atoms(32, 3, 124, 72, mode) + (size_t)125 * 256);
    expect_size("beyond the cap", impnn_encoder_prepared_bytes_gates(32, 3, 300, 72, mode), old);
    expect_size("no steps", impnn_encoder_prepared_bytes_gates(32, 0, 124, 72, mode), impnn_encoder_prepared_bytes(32, 0, 72, mode));
    const size_t old64 = impnn_encoder_prepared_bytes(32, 3, 64, mode);
    expect_size("at the cap", impnn_encoder_prepared_bytes_gates(32, 3, 255, 64, mode), old64 + ((size_t)2 << 20) + (size_t)256 * 256);
    expect_size("one column more", impnn_encoder_prepared_bytes_gates(32, 3, 256, 64, mode), old64);
    expect_size("the with-atoms size is unchanged", impnn_encoder_prepared_bytes_atoms(32, 3, 124, 72, mode), old + (size_t)72 * 125 * 128);
  }
  expect_size("pull mode", impnn_encoder_prepared_bytes_gates(32, 3, 124, 72, IMPNN_ENCODER_F32), impnn_encoder_prepared_bytes(32, 3, 72, IMPNN_ENCODER_F32));
  expect_size("wide states", impnn_encoder_prepared_bytes_gates(128, 3, 124, 72, IMPNN_ENCODER_F32_TYPED),
              impnn_encoder_prepared_bytes(128, 3, 72, IMPNN_ENCODER_F32_TYPED));
  expect_size("atom_dim 48", impnn_encoder_prepared_bytes_gates(48, 3, 124, 72, IMPNN_ENCODER_F32_TYPED), 0);
  expect_size("Va = 0", impnn_encoder_prepared_bytes_gates(32, 3, 0, 72, IMPNN_ENCODER_F32_TYPED), 0);
  expect_size("Va < 0", impnn_encoder_prepared_bytes_gates(32, 3, -7, 72, IMPNN_ENCODER_F32_TYPED), 0);
  expect_size("mode 4", impnn_encoder_prepared_bytes_gates(32, 3, 124, 72, 4), 0);
  expect_size("huge Va", impnn_encoder_prepared_bytes_gates(32, 3, 0x7fffffff, 256, IMPNN_ENCODER_F32_TYPED),
              impnn_encoder_prepared_bytes(32, 3, 256, IMPNN_ENCODER_F32_TYPED));

  // ---- the prepare entry
  for (int mode = IMPNN_ENCODER_F32_TYPED; mode <= IMPNN_ENCODER_F32X3_TYPED; ++mode) {
#define BAD(code, stmt)         \
  do {                          \
    Args a;                     \
    a.mode = mode;              \
    stmt;                       \
    expect(#stmt, call(a), code); \
  } while (0)
    BAD(IMPNN_E_BADARG, a.weights = nullptr);
    BAD(IMPNN_E_BADARG, a.bond_table = nullptr);
    BAD(IMPNN_E_BADARG, a.atom_table = nullptr);
    BAD(IMPNN_E_BADARG, a.prepared = nullptr);
    BAD(IMPNN_E_BADARG, a.prepared = at<void>(0x200008));
    BAD(IMPNN_E_BADARG, a.atom_table = at<float>(0x100004));
    BAD(IMPNN_E_BADARG, a.Va = 0);
    BAD(IMPNN_E_BADARG, a.Va = -1);
    BAD(IMPNN_E_BADARG, a.Vb = 0);
    BAD(IMPNN_E_BADARG, a.K = 0);
    BAD(IMPNN_E_BADARG, a.D = 0);
    BAD(IMPNN_E_BADARG, a.S = -1);
    BAD(IMPNN_E_UNSUPPORTED, a.D = 48);
    BAD(IMPNN_E_UNSUPPORTED, a.Vb = 257);
    BAD(IMPNN_E_WORKSPACE, a.bytes = 0);
    BAD(IMPNN_E_WORKSPACE, a.bytes = impnn_encoder_prepared_bytes(32, 3, 72, mode));  // the image alone
    BAD(IMPNN_E_WORKSPACE, a.bytes = impnn_encoder_prepared_bytes_atoms(32, 3, 124, 72, mode));  // no room for the gate table
    BAD(IMPNN_E_WORKSPACE, a.bytes = impnn_encoder_prepared_bytes_gates(32, 3, 124, 72, mode) - 1);
    BAD(IMPNN_E_WORKSPACE, (a.Va = 300, a.bytes = impnn_encoder_prepared_bytes(32, 3, 72, mode) - 1));  // beyond the cap
    BAD(IMPNN_OK, (a.S = 0, a.weights = nullptr, a.prepared = nullptr, a.bytes = 0));  // nothing to build
#undef BAD
  }
  {
    Args a;
    a.mode = 4;
    expect("mode 4", call(a), IMPNN_E_BADARG);
    a.mode = IMPNN_ENCODER_F32;
    a.atom_table = nullptr;
    expect("pull mode, null atom_table", call(a), IMPNN_E_BADARG);
  }
  if (std::strstr(impnn_last_error_string(), "null") == nullptr) ++failures, std::printf("FAIL: last error text\n");
  std::printf(failures ? "%d FAILURES\n" : "prepare_gates_args_check: all refusals as specified\n", failures);
  return failures ? 1 : 0;
}
