// extern "C" boundary of libimpnn.so: argument checks, then launches.  See include/impnn.h.
#include <cstring>
#include <vector>

#include <cstddef>

#include "common.h"
#include "encoder_layout.h"

namespace impnn {

char* error_buffer() {
  static thread_local char buf[512] = {0};
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(error_buffer(), 512, fmt, ap);
  va_end(ap);
  return code;
}

namespace {
struct Profiler {
  std::vector<hipEvent_t> start, stop;
  int used = 0;
  bool enabled = false;
  bool open = false;  // a start without its stop
};
thread_local Profiler g_prof;
}  // namespace

namespace {
thread_local void* g_stamp_ptr = nullptr;
thread_local size_t g_stamp_bytes = 0;
}  // namespace

void* debug_stamp_buffer(size_t* bytes) {
  *bytes = g_stamp_bytes;
  return g_stamp_ptr;
}

void profile_record_start(hipStream_t s) {
  Profiler& p = g_prof;
  if (!p.enabled || p.used >= (int)p.start.size()) return;
  if (hipEventRecord(p.start[p.used], s) == hipSuccess) p.open = true;
}

void profile_record_stop(hipStream_t s) {
  Profiler& p = g_prof;
  if (!p.enabled || !p.open) return;
  (void)hipEventRecord(p.stop[p.used], s);
  p.open = false;
  ++p.used;
}

}  // namespace impnn

using namespace impnn;

#define REQUIRE(cond, what)                                              \
  do {                                                                   \
    if (!(cond)) return fail(IMPNN_E_BADARG, "%s: %s", __func__, what); \
  } while (0)

// ---- the GatedUpdate family (include/impnn.h).  Each entry fills a GatedUpdateCall with its form; one check per
// direction applies the family's rules in a fixed order and launches.
namespace {

constexpr GuArg kNo = GuArg::kAbsent, kOpt = GuArg::kOptional, kReq = GuArg::kRequired;
// impnn_gated_update(_dropout), _rows, _rows_train, _rows_train_dropout (rate > 0); a forward row list's atom_dims
// (32, 64, 128) are checked after its arguments
constexpr GatedUpdateForm kFwd{kNo, kNo, GuDims::kAny}, kFwdRows{kReq, kNo, GuDims::kAny},
    kFwdTrain{kOpt, kReq, GuDims::k32_64_128}, kFwdTrainDropout{kOpt, kOpt, GuDims::kAny};
// impnn_gated_update_bwd, _rows_bwd, _rows_bwd_saved, each with its _dropout twin
constexpr GatedUpdateForm kBwd{kNo, kNo, GuDims::kDivide256}, kBwdRows{kReq, kNo, GuDims::k64_128},
    kBwdSaved{kOpt, kReq, GuDims::k32_64_128};

bool covers(GuDims dims, int D) {
  switch (dims) {
    case GuDims::kAny: return D > 0;
    case GuDims::kDivide256: return D > 0 && D <= 256 && 256 % D == 0;
    case GuDims::k32_64_128: return D == 32 || D == 64 || D == 128;
    case GuDims::k64_128: return D == 64 || D == 128;
  }
  return false;
}

int uncovered(const GatedUpdateCall& c, const char* what) {
  return fail(IMPNN_E_UNSUPPORTED, "%s: atom_dim %d (%s)", c.entry, c.D, what);
}

#define CHECK(cond, what)                                                  \
  do {                                                                     \
    if (!(cond)) return fail(IMPNN_E_BADARG, "%s: %s", c.entry, what);   \
  } while (0)

// rows >= 0 and the form's atom_dims: an open rule (any, divides 256) is part of the shape, a fixed set is coverage
int check_shape(const GatedUpdateCall& c) {
  const GuDims dims = c.form.dims;
  const bool open = dims == GuDims::kAny || dims == GuDims::kDivide256;
  CHECK(c.rows >= 0 && (!open || covers(dims, c.D)), dims == GuDims::kDivide256 ? "atom_dim must divide 256" : "bad shape");
  if (!covers(dims, c.D))
    return uncovered(c, dims == GuDims::k64_128 ? "the row-list form covers 64 and 128" : "the saving form covers 32, 64 and 128");
  return IMPNN_OK;
}

// a form without a row list or a saved buffer leaves those pointers null
void clear_absent(GatedUpdateCall& c) {
  if (c.form.row_list == kNo) c.row_index = c.n_rows = nullptr;
  if (c.form.saved == kNo) c.saved = nullptr;
}

int gated_update_checked(GatedUpdateCall c) {
  clear_absent(c);
  if (int rc = check_shape(c)) return rc;
  if (c.saved && !covers(GuDims::k32_64_128, c.D)) return uncovered(c, "the saving forward covers 32, 64 and 128");
  if (c.rows == 0) return IMPNN_OK;
  CHECK(c.h && c.agg && c.Wz && c.bz && c.Wr && c.br && c.Wh && c.bh && c.gamma && c.beta && c.out &&
            (c.form.row_list != kReq || (c.row_index && c.n_rows)) && (c.form.saved != kReq || c.saved),
        "null pointer");
  CHECK((c.row_index != nullptr) == (c.n_rows != nullptr), "row_index and n_rows: both or neither");
  CHECK(!c.saved || aligned16(c.saved), "saved must be 16-byte aligned");
  CHECK(c.eps >= 0.f, "ln_eps must be >= 0");
  if (c.row_index && !covers(GuDims::k32_64_128, c.D)) return uncovered(c, "a row list covers 32, 64 and 128");
  CHECK(c.D != 32 || !(c.row_index || c.saved) || (aligned16(c.h) && aligned16(c.agg) && aligned16(c.out)),
        "a row list or saved buffer at atom_dim 32 needs 16-byte aligned tensors");
  return launch_gated_update(c);
}

int gated_update_bwd_checked(GatedUpdateCall c) {
  clear_absent(c);
  if (int rc = check_shape(c)) return rc;
  CHECK(c.h && c.agg && c.Wz && c.bz && c.Wr && c.br && c.Wh && c.bh && c.gamma && c.dout && c.dh && c.dagg &&
            c.dparams && c.workspace && (c.form.row_list != kReq || (c.row_index && c.n_rows)) &&
            (c.form.saved != kReq || c.saved),
        "null pointer");
  CHECK((c.row_index != nullptr) == (c.n_rows != nullptr), "row_index and n_rows: both or neither");
  if (c.row_index && !covers(GuDims::k64_128, c.D)) return uncovered(c, "a row list covers 64 and 128");
  // the forms that take a row list size their workspace for one (impnn_gated_update_rows_bwd_workspace_floats) where
  // it exists, at atom_dim 64 / 128, list or not
  const bool list_ws = c.form.row_list != kNo && covers(GuDims::k64_128, c.D);
  if (c.workspace_floats < gated_update_bwd_workspace(c.rows, c.D, list_ws))
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %lld floats is too small", c.entry, (long long)c.workspace_floats);
  // zero rows: the plain form still writes dparams (zeros, or nothing added)
  if (c.rows == 0 && (c.form.row_list != kNo || c.form.saved != kNo)) return IMPNN_OK;
  CHECK(!(c.row_index || c.saved) || (aligned16(c.h) && aligned16(c.agg) && aligned16(c.dout) && aligned16(c.dh) &&
                                      aligned16(c.dagg) && aligned16(c.workspace) && (!c.saved || aligned16(c.saved))),
        "the row-list and saving forms need 16-byte aligned tensors");
  return launch_gated_update_bwd(c);
}
#undef CHECK

int check_dropout(const char* entry, float rate, uint64_t seed, const int64_t* step, int32_t layer_word,
                  DropoutArgs* d) {
  if (!step) return fail(IMPNN_E_BADARG, "%s: null step pointer", entry);
  if (!dropout_args(rate, seed, step, layer_word, d))
    return fail(IMPNN_E_BADARG, "%s: dropout rate %g is not in [0, 1)", entry, (double)rate);
  return IMPNN_OK;
}

// a *_dropout entry's tail, checked before everything else; rate 0 is the plain entry's call
int add_dropout(GatedUpdateCall& c, float rate, uint64_t seed, const int64_t* step, int32_t layer_word) {
  c.dropout = rate != 0.f;
  return check_dropout(c.entry, rate, seed, step, layer_word, &c.drop);
}

GatedUpdateCall gu_forward(const char* entry, GatedUpdateForm form, const float* h, const float* agg, const float* Wz,
                           const float* bz, const float* Wr, const float* br, const float* Wh, const float* bh,
                           const float* gamma, const float* beta, float eps, float* out, const int32_t* row_index,
                           const int32_t* n_rows, int64_t rows, int32_t D, float* saved, impnn_stream_t stream) {
  GatedUpdateCall c{};
  c.entry = entry, c.form = form, c.h = h, c.agg = agg, c.Wz = Wz, c.bz = bz, c.Wr = Wr, c.br = br, c.Wh = Wh;
  c.bh = bh, c.gamma = gamma, c.beta = beta, c.eps = eps, c.out = out;
  c.row_index = row_index, c.n_rows = n_rows, c.rows = rows, c.D = D, c.saved = saved, c.stream = as_stream(stream);
  return c;
}

GatedUpdateCall gu_backward(const char* entry, GatedUpdateForm form, const float* h, const float* agg,
                            const float* Wz, const float* bz, const float* Wr, const float* br, const float* Wh,
                            const float* bh, const float* gamma, float eps, const float* dout, float* dh, float* dagg,
                            float* dparams, float* workspace, int64_t workspace_floats, const int32_t* row_index,
                            const int32_t* n_rows, int64_t rows, int32_t D, int32_t accumulate, float* saved,
                            impnn_stream_t stream) {
  GatedUpdateCall c{};
  c.entry = entry, c.form = form, c.h = h, c.agg = agg, c.Wz = Wz, c.bz = bz, c.Wr = Wr, c.br = br, c.Wh = Wh;
  c.bh = bh, c.gamma = gamma, c.eps = eps, c.dout = dout, c.dh = dh, c.dagg = dagg, c.dparams = dparams;
  c.workspace = workspace, c.workspace_floats = workspace_floats, c.accumulate = accumulate != 0;
  c.row_index = row_index, c.n_rows = n_rows, c.rows = rows, c.D = D, c.saved = saved, c.stream = as_stream(stream);
  return c;
}

// ---- the typed-message family (include/impnn.h; message_typed.hip).  Each entry fills a TypedMessageCall; one check
// applies the family's rules in a fixed order and launches.
TypedMessageCall typed_message(const char* entry, const float* h, const int32_t* bond_ids, const int32_t* conn,
                               const float* type_mats, void* workspace, int64_t workspace_bytes, int32_t B, int32_t N,
                               int32_t E, int32_t D, int32_t Vb, int32_t sort_ready, impnn_stream_t stream) {
  TypedMessageCall c{};
  c.entry = entry, c.h = h, c.bond_ids = bond_ids, c.conn = conn, c.type_mats = type_mats, c.workspace = workspace;
  c.workspace_bytes = workspace_bytes, c.B = B, c.N = N, c.E = E, c.D = D, c.Vb = Vb, c.sort_ready = sort_ready != 0;
  c.stream = as_stream(stream);
  return c;
}

// The family's rules in their order: shape, zero work, null pointers (`tensors`: the entry's own are non-null), workspace
// size, coverage - then the launch (the adjoint's refuses a misaligned edge buffer before it launches anything).
int typed_message_checked(const TypedMessageCall& c, bool tensors, int (*launch)(const TypedMessageCall&)) {
  if (!(c.B >= 0 && c.N > 0 && c.E >= 0 && c.D > 0 && c.Vb > 0)) return fail(IMPNN_E_BADARG, "%s: bad shape", c.entry);
  if (c.B == 0 || c.E == 0) return IMPNN_OK;
  if (!(c.h && c.bond_ids && c.conn && c.type_mats && c.workspace && tensors))
    return fail(IMPNN_E_BADARG, "%s: null pointer", c.entry);
  if (c.workspace_bytes < 4 * bmm_message_typed_bwd_workspace_ints(c.B, c.E, c.Vb))
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %lld bytes is too small", c.entry, (long long)c.workspace_bytes);
  if (c.Vb > kMaxTypes) return fail(IMPNN_E_UNSUPPORTED, "%s: Vb=%d too large", c.entry, c.Vb);
  if (c.D > 128) return fail(IMPNN_E_UNSUPPORTED, "%s: D=%d > 128", c.entry, c.D);
  return launch(c);
}

// ---- the model head family (include/impnn.h; model_head.hip).  Each entry fills a ModelHeadCall; one check applies the
// family's rules in a fixed order and launches.
ModelHeadCall model_head(const char* entry, int32_t kind, const float* pooled_cat, const float* pooled_an,
                         const float* temperature, int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  ModelHeadCall c{};
  c.entry = entry, c.kind = kind, c.pc = pooled_cat, c.pa = pooled_an, c.T = temperature;
  c.B = B, c.D = D, c.F = F, c.Mx = Mx, c.stream = as_stream(stream);
  return c;
}

struct ModelHeadForm {
  bool empty_batch, tensors;  // B == 0 is a success (not for the loss entries); the entry's own pointers are non-null
  int (*launch)(const ModelHeadCall&);
};

// The family's rules in their order: kind, shape, zero work, null pointers (the temperature is kind 0's alone), workspace
// size (the loss forward is the one entry with a workspace) - then the launcher: widths, null weight / gradient tensor
// i, LDS fit.
int model_head_checked(const ModelHeadCall& c, ModelHeadForm form) {
  if (!(c.kind == 0 || c.kind == 1))
    return fail(IMPNN_E_BADARG, "%s: kind must be 0 (viscosity) or 1 (melting point)", c.entry);
  if (!(c.B >= (form.empty_batch ? 0 : 1) && c.D > 0 && c.F > 0 && c.Mx > 0))
    return fail(IMPNN_E_BADARG, "%s: bad shape", c.entry);
  if (c.B == 0) return IMPNN_OK;
  if (!(c.pc && c.pa && form.tensors && (c.kind == 1 || c.T))) return fail(IMPNN_E_BADARG, "%s: null pointer", c.entry);
  if (reinterpret_cast<uintptr_t>(c.sample_weight) % sizeof(float))
    return fail(IMPNN_E_BADARG, "%s: sample_weight must be 4-byte aligned", c.entry);
  if (c.workspace && c.workspace_floats < impnn_model_head_loss_workspace_floats(c.B))
    return fail(IMPNN_E_WORKSPACE, "model_head_loss: workspace of %lld floats is too small", (long long)c.workspace_floats);
  return form.launch(c);
}

}  // namespace

extern "C" {

int impnn_abi_version(void) { return IMPNN_ABI_VERSION; }
const char* impnn_last_error_string(void) { return error_buffer(); }
const char* impnn_target_arch(void) { return "gfx950"; }

int impnn_embed_gather(const int32_t* ids, const float* table, float* out, int64_t rows, int32_t vocab,
                       int32_t dim, impnn_stream_t stream) {
  REQUIRE(rows >= 0 && vocab > 0 && dim > 0, "rows>=0, vocab>0, dim>0 required");
  REQUIRE(rows == 0 || (ids && table && out), "null pointer");
  return launch_embed_gather(ids, table, out, rows, vocab, dim, as_stream(stream));
}

int impnn_bmm_message(const float* h, const float* bond_state, const int32_t* conn, const float* W,
                      float* messages, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                      impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E >= 0 && D > 0 && K > 0, "bad shape");
  if (B == 0 || E == 0) return IMPNN_OK;
  REQUIRE(h && bond_state && conn && W && messages, "null pointer");
  return launch_bmm_message(h, bond_state, conn, W, messages, nullptr, B, N, E, D, K, as_stream(stream));
}

int impnn_bond_type_matrices(const float* bond_table, const float* W, float* out, int32_t Vb, int32_t K,
                             int32_t D, impnn_stream_t stream) {
  REQUIRE(Vb > 0 && K > 0 && D > 0, "bad shape");
  REQUIRE(bond_table && W && out, "null pointer");
  return launch_bond_type_matrices(bond_table, W, out, Vb, K, D, as_stream(stream));
}

int impnn_bmm_message_typed(const float* h, const int32_t* bond_ids, const int32_t* conn,
                            const float* type_mats, float* messages, int32_t B, int32_t N, int32_t E,
                            int32_t D, int32_t Vb, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E >= 0 && D > 0 && Vb > 0, "bad shape");
  if (B == 0 || E == 0) return IMPNN_OK;
  REQUIRE(h && bond_ids && conn && type_mats && messages, "null pointer");
  return launch_bmm_message_typed(h, bond_ids, conn, type_mats, messages, B, N, E, D, Vb, as_stream(stream));
}

int impnn_reduce_scatter_add(const float* messages, const int32_t* tgt, int32_t tgt_stride, float* agg,
                             int32_t B, int32_t N, int32_t E, int32_t D, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E >= 0 && D > 0, "bad shape");
  REQUIRE(tgt_stride >= 1, "tgt_stride must be >= 1");
  if (B == 0) return IMPNN_OK;
  REQUIRE(agg && (E == 0 || (messages && tgt)), "null pointer");
  return launch_reduce_scatter_add(messages, tgt, tgt_stride, agg, B, N, E, D, as_stream(stream));
}

int impnn_bmm_fused(const float* h, const float* bond_state, const int32_t* conn, const float* W, float* agg,
                    int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E > 0 && D > 0 && K > 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(h && bond_state && conn && W && agg, "null pointer");
  return launch_bmm_message(h, bond_state, conn, W, nullptr, agg, B, N, E, D, K, as_stream(stream));
}

int impnn_kept_rows(const int32_t* atom_ids, const int32_t* bond_ids, const int32_t* conn, int32_t* rows_out,
                    int32_t B, int32_t N, int32_t E, int32_t Vb, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E >= 0 && Vb > 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(atom_ids && rows_out && (E == 0 || conn), "null pointer");
  return launch_kept_rows(atom_ids, bond_ids, conn, rows_out, B, N, E, Vb, as_stream(stream));
}

int impnn_row_index_fill(const int32_t* kept_rows, const int32_t* kept_rows_inclusive_prefix, int32_t* row_index,
                         int32_t* n_rows, int32_t B, int32_t N, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(kept_rows && kept_rows_inclusive_prefix && row_index && n_rows, "null pointer");
  return launch_row_index_fill(kept_rows, kept_rows_inclusive_prefix, row_index, n_rows, B, N, as_stream(stream));
}

int impnn_global_sum_pool(const float* h, const int32_t* atom_ids, float* out, int32_t B, int32_t N,
                          int32_t D, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && D > 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(h && atom_ids && out, "null pointer");
  return launch_global_sum_pool(h, atom_ids, out, B, N, D, as_stream(stream));
}

size_t impnn_encoder_plan_overflow_offset(void) { return offsetof(enc::PlanHeader, overflow); }

int64_t impnn_encoder_step_floats(int32_t D, int32_t K) {
  if (D <= 0 || K <= 0) return -1;
  const int64_t d = D, k = K;
  return k * d * d + 3 * (2 * d * d + d) + 2 * d;
}

namespace {
constexpr int32_t kInfoMagic = 0x706c616e;  // "plan"
// impnn_encoder_plan_info.v: magic, mode class (0 pull records / 1 typed records), n_ions, B, N, E, S, Vb, nwg, D, K,
// record kind (0 pull, 1 typed atom_dim 32, 2 wide atom_dim 64 / 128: three different workspace layouts)
inline int mode_class(int mode) { return mode >= 2 ? 1 : 0; }
inline int record_kind(int mode, int D) { return mode >= 2 ? (D == 32 ? 1 : 2) : 0; }
}  // namespace

int impnn_encoder_workspace_bytes(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                                  int32_t S, int32_t Vb, int32_t mode, int32_t workgroups, size_t* bytes) {
  REQUIRE(bytes, "null pointer");
  REQUIRE(n_ions >= 1 && n_ions <= 2 && B >= 0 && N > 0 && E >= 0 && D > 0 && K > 0 && S >= 0 && Vb > 0,
          "bad shape");
  REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (f32), 1 (f16x2), 2 (f32 typed) or 3 (f32x3 typed)");
  REQUIRE(workgroups >= 0, "workgroups must be >= 0 (0: default)");
  if (!encoder_fused_supported(mode, N, E, D, K, S, Vb))
    return fail(IMPNN_E_UNSUPPORTED, "encoder_fused: mode=%d shape N=%d E=%d D=%d K=%d S=%d Vb=%d not covered", mode,
                N, E, D, K, S, Vb);
  if (D != enc::kD && !encoder_wide_batch_covered(n_ions, B, N, E, D, Vb))  // before anything is allocated for it
    return fail(IMPNN_E_UNSUPPORTED, "encoder_fused: batch of %d pairs x (N=%d, E=%d) at D=%d exceeds 32-bit row / edge "
                "indices or row offsets: split the batch", B, N, E, D);
  *bytes = encoder_fused_workspace_bytes(mode, n_ions, B, N, E, D, S, Vb, encoder_workgroups(n_ions, B, workgroups, N, E, mode));
  return IMPNN_OK;
}

// Where the plan of such a call lies in its workspace (atom_dim 32): the same functions the plan and the run size and
// address it with (encoder_workgroups, enc::ws_layout, enc::plan_vmin).  Host arithmetic only.
int impnn_encoder_plan_layout(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, int32_t S,
                              int32_t Vb, int32_t mode, int32_t workgroups, int64_t out[8]) {
  REQUIRE(out, "null pointer");
  size_t total = 0;
  if (int rc = impnn_encoder_workspace_bytes(n_ions, B, N, E, D, K, S, Vb, mode, workgroups, &total)) return rc;
  if (D != enc::kD)
    return fail(IMPNN_E_UNSUPPORTED, "encoder_plan_layout: atom_dim %d has no chunk plan (atom_dim 32 only)", D);
  const bool typed = mode >= 2;
  const int nwg = encoder_workgroups(n_ions, B, workgroups, N, E, mode);
  const enc::Ws w = enc::ws_layout(n_ions, B, N, E, S, Vb, nwg, typed, mode == 3);
  out[0] = w.nwg;
  out[1] = w.max_sub;
  out[2] = (int64_t)w.rows_off;
  out[3] = (int64_t)w.vr_off;
  out[4] = (int64_t)w.nsub_off;
  out[5] = (int64_t)w.desc_off;
  out[6] = typed ? enc::tecap_of(E) : 0;
  out[7] = enc::plan_vmin(n_ions, B, enc::vr_max_of(N, E, typed), w.nwg);
  return IMPNN_OK;
}

// Where the chunk records of such a call lie (typed modes, atom_dim 32).  Host arithmetic only.
int impnn_encoder_plan_records(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, int32_t S,
                               int32_t Vb, int32_t mode, int32_t workgroups, int64_t out[5]) {
  REQUIRE(out, "null pointer");
  size_t total = 0;
  if (int rc = impnn_encoder_workspace_bytes(n_ions, B, N, E, D, K, S, Vb, mode, workgroups, &total)) return rc;
  if (D != enc::kD)
    return fail(IMPNN_E_UNSUPPORTED, "encoder_plan_records: atom_dim %d has no chunk plan (atom_dim 32 only)", D);
  if (mode < 2)
    return fail(IMPNN_E_UNSUPPORTED, "encoder_plan_records: mode %d has pull-form records (typed modes only)", mode);
  const int nwg = encoder_workgroups(n_ions, B, workgroups, N, E, mode);
  const enc::Ws w = enc::ws_layout(n_ions, B, N, E, S, Vb, nwg, true, mode == 3);
  out[0] = (int64_t)w.rec_off;
  out[1] = w.rec_bytes;
  out[2] = enc::kTRecGrp;
  out[3] = enc::trec_runs_off(Vb, enc::tecap_of(E));
  out[4] = enc::kTRecNrun;
  return IMPNN_OK;
}

static int encoder_common(const char* fn, int32_t n_ions, const int32_t* const* atom_ids,
                          const int32_t* const* bond_ids, const int32_t* const* conn, const float* atom_table,
                          int32_t Va, const float* bond_table, int32_t Vb, const float* const* weights,
                          const void* const* prepared, int32_t mode, float* const* pooled, int32_t B, int32_t N,
                          int32_t E, int32_t D, int32_t K, int32_t S, float ln_eps, int32_t workgroups,
                          const impnn_encoder_plan_info* info_in, impnn_encoder_plan_info* info_out, void* workspace,
                          size_t workspace_bytes, impnn_stream_t stream, int phases = 3) {
#define REQ(cond, what)                                           \
  do {                                                            \
    if (!(cond)) return fail(IMPNN_E_BADARG, "%s: %s", fn, what); \
  } while (0)
  REQ(n_ions >= 1 && n_ions <= 2, "n_ions must be 1 or 2");
  REQ(mode >= 0 && mode <= 3, "mode must be 0 (f32), 1 (f16x2), 2 (f32 typed) or 3 (f32x3 typed)");
  REQ(workgroups >= 0, "workgroups must be >= 0 (0: default)");
  REQ(B >= 0 && N > 0 && E >= 0 && D > 0 && K > 0 && S >= 0 && Va > 0 && Vb > 0, "bad shape");
  const bool planning = (phases & 1) != 0, running = (phases & 2) != 0;
  REQ(atom_ids && (!planning || (bond_ids && conn)), "null pointer");
  REQ(!running || ((weights || prepared) && pooled && atom_table && bond_table), "null pointer");
  if (!encoder_fused_supported(mode, N, E, D, K, S, Vb))
    return fail(IMPNN_E_UNSUPPORTED, "encoder_fused: mode=%d shape N=%d E=%d D=%d K=%d S=%d Vb=%d not covered", mode,
                N, E, D, K, S, Vb);
  int nwg = encoder_workgroups(n_ions, B, workgroups, N, E, mode);
  if (info_in) {  // run half: the plan's geometry is authoritative, and must be the geometry of this call
    const int32_t* v = info_in->v;
    REQ(v[0] == kInfoMagic, "plan info was not filled by impnn_encoder_plan");
    if (v[1] != mode_class(mode) || v[2] != n_ions || v[3] != B || v[4] != N || v[5] != E || v[6] != S || v[7] != Vb ||
        v[9] != D || v[10] != K || v[11] != record_kind(mode, D))
      return fail(IMPNN_E_BADARG, "%s: the workspace was planned for another batch shape or record kind "
                  "(planned: kind %d/%d, n_ions %d, B %d, N %d, E %d, S %d, Vb %d, D %d, K %d)", fn, v[1], v[11], v[2],
                  v[3], v[4], v[5], v[6], v[7], v[9], v[10]);
    nwg = v[8];
  }
  if (info_out) {
    int32_t* v = info_out->v;
    for (int i = 0; i < 12; ++i) v[i] = 0;
    v[0] = kInfoMagic; v[1] = mode_class(mode); v[2] = n_ions; v[3] = B; v[4] = N; v[5] = E; v[6] = S; v[7] = Vb;
    v[8] = nwg; v[9] = D; v[10] = K; v[11] = record_kind(mode, D);
  }
  if (B == 0) return IMPNN_OK;
  EncoderArgs a{};
  a.n_ions = n_ions;
  a.mode = mode;
  a.phases = phases;
  a.nwg = nwg;
  for (int g = 0; g < n_ions; ++g) {
    const bool have_w = !running || S == 0 || (prepared && prepared[g]) || (weights && weights[g]);
    REQ(atom_ids[g] && have_w, "null per-ion pointer");
    REQ(!planning || E == 0 || (bond_ids[g] && conn[g]), "null per-ion pointer");
    REQ(!running || pooled[g], "null per-ion pointer");
    a.atom_ids[g] = atom_ids[g];
    a.bond_ids[g] = bond_ids ? bond_ids[g] : nullptr;
    a.conn[g] = conn ? conn[g] : nullptr;
    a.weights[g] = weights ? weights[g] : nullptr;
    a.prepared[g] = prepared ? prepared[g] : nullptr;
    a.pooled[g] = pooled ? pooled[g] : nullptr;
  }
#undef REQ
  a.atom_table = atom_table;
  a.bond_table = bond_table;
  a.Va = Va; a.Vb = Vb; a.B = B; a.N = N; a.E = E; a.D = D; a.K = K; a.S = S;
  a.ln_eps = ln_eps;
  a.workspace = workspace;
  a.workspace_bytes = workspace_bytes;
  const size_t need = encoder_fused_workspace_bytes(mode, n_ions, B, N, E, D, S, Vb, nwg);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return fail(IMPNN_E_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
  return launch_encoder_fused(a, as_stream(stream));
}

int impnn_encoder_fused(int32_t n_ions, const int32_t* const* atom_ids, const int32_t* const* bond_ids,
                        const int32_t* const* conn, const float* atom_table, int32_t Va,
                        const float* bond_table, int32_t Vb, const float* const* weights, int32_t mode,
                        float* const* pooled, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, int32_t S,
                        float ln_eps, int32_t workgroups, void* workspace, size_t workspace_bytes,
                        impnn_stream_t stream) {
  return encoder_common(__func__, n_ions, atom_ids, bond_ids, conn, atom_table, Va, bond_table, Vb, weights, nullptr,
                        mode, pooled, B, N, E, D, K, S, ln_eps, workgroups, nullptr, nullptr, workspace,
                        workspace_bytes, stream);
}

int impnn_encoder_plan(int32_t n_ions, const int32_t* const* atom_ids, const int32_t* const* bond_ids,
                       const int32_t* const* conn, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, int32_t S,
                       int32_t Va, int32_t Vb, int32_t mode, int32_t workgroups, void* workspace,
                       size_t workspace_bytes, impnn_stream_t stream, impnn_encoder_plan_info* info) {
  REQUIRE(info, "null plan info");
  return encoder_common(__func__, n_ions, atom_ids, bond_ids, conn, nullptr, Va, nullptr, Vb, nullptr, nullptr, mode,
                        nullptr, B, N, E, D, K, S, 0.f, workgroups, nullptr, info, workspace, workspace_bytes, stream,
                        1);
}

int impnn_encoder_run(int32_t n_ions, const int32_t* const* atom_ids, const float* atom_table, int32_t Va,
                      const float* bond_table, int32_t Vb, const void* const* prepared, int32_t mode,
                      float* const* pooled, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K, int32_t S,
                      float ln_eps, const impnn_encoder_plan_info* info, void* workspace, size_t workspace_bytes,
                      impnn_stream_t stream) {
  REQUIRE(info, "null plan info");
  return encoder_common(__func__, n_ions, atom_ids, nullptr, nullptr, atom_table, Va, bond_table, Vb, nullptr,
                        prepared, mode, pooled, B, N, E, D, K, S, ln_eps, 0, info, nullptr, workspace,
                        workspace_bytes, stream, 2);
}

size_t impnn_encoder_prepared_bytes(int32_t D, int32_t S, int32_t Vb, int32_t mode) {
  if (mode < 0 || mode > 3 || Vb <= 0 || D <= 0) return 0;
  if (!encoder_fused_supported(mode, 1, 0, D, 1, S, mode >= 2 ? Vb : 1)) return 0;
  return encoder_prepared_bytes(mode, D, S, Vb);
}

int impnn_encoder_prepare_weights(const float* weights, const float* bond_table, int32_t D, int32_t K, int32_t S,
                                  int32_t Vb, int32_t mode, void* prepared, size_t prepared_bytes,
                                  impnn_stream_t stream) {
  REQUIRE(D > 0 && K > 0 && S >= 0 && Vb > 0, "bad shape");
  REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (f32), 1 (f16x2), 2 (f32 typed) or 3 (f32x3 typed)");
  if (!encoder_fused_supported(mode, 1, 0, D, K, S, mode >= 2 ? Vb : 1))
    return fail(IMPNN_E_UNSUPPORTED, "encoder_prepare_weights: mode=%d D=%d K=%d Vb=%d not covered", mode, D, K, Vb);
  if (S == 0) return IMPNN_OK;
  REQUIRE(weights && prepared && (mode < 2 || bond_table), "null pointer");
  REQUIRE(aligned16(prepared), "prepared buffer must be 16B aligned");
  if (prepared_bytes < encoder_prepared_bytes(mode, D, S, Vb))
    return fail(IMPNN_E_WORKSPACE, "encoder_prepare_weights: buffer %zu < %zu bytes", prepared_bytes,
                encoder_prepared_bytes(mode, D, S, Vb));
  return launch_encoder_prepare(weights, bond_table, D, K, S, Vb, mode, prepared, as_stream(stream));
}

size_t impnn_encoder_prepared_bytes_atoms(int32_t D, int32_t S, int32_t Va, int32_t Vb, int32_t mode) {
  if (Va <= 0 || impnn_encoder_prepared_bytes(D, S, Vb, mode) == 0) return 0;
  return encoder_prepared_bytes_atoms(mode, D, S, Va, Vb);
}

int impnn_encoder_prepare_weights_atoms(const float* weights, const float* bond_table, const float* atom_table,
                                        int32_t Va, int32_t D, int32_t K, int32_t S, int32_t Vb, int32_t mode,
                                        void* prepared, size_t prepared_bytes, impnn_stream_t stream) {
  REQUIRE(D > 0 && K > 0 && S >= 0 && Vb > 0 && Va > 0, "bad shape");
  REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (f32), 1 (f16x2), 2 (f32 typed) or 3 (f32x3 typed)");
  if (!encoder_fused_supported(mode, 1, 0, D, K, S, mode >= 2 ? Vb : 1))
    return fail(IMPNN_E_UNSUPPORTED, "encoder_prepare_weights_atoms: mode=%d D=%d K=%d Vb=%d not covered", mode, D, K, Vb);
  if (S == 0) return IMPNN_OK;
  REQUIRE(weights && prepared && atom_table && (mode < 2 || bond_table), "null pointer");
  REQUIRE(aligned16(prepared) && aligned16(atom_table), "prepared buffer and atom_table must be 16B aligned");
  if (prepared_bytes < encoder_prepared_bytes_atoms(mode, D, S, Va, Vb))
    return fail(IMPNN_E_WORKSPACE, "encoder_prepare_weights_atoms: buffer %zu < %zu bytes", prepared_bytes,
                encoder_prepared_bytes_atoms(mode, D, S, Va, Vb));
  return launch_encoder_prepare_atoms(weights, bond_table, atom_table, Va, D, K, S, Vb, mode, prepared, as_stream(stream));
}

size_t impnn_encoder_prepared_bytes_gates(int32_t D, int32_t S, int32_t Va, int32_t Vb, int32_t mode) {
  const size_t atoms = impnn_encoder_prepared_bytes_atoms(D, S, Va, Vb, mode);
  if (atoms == 0) return 0;
  const size_t gates = encoder_prepared_bytes_gates(mode, D, S, Va, Vb);
  return gates > atoms ? (gates + 15) & ~(size_t)15 : atoms;  // no gate table: the with-atoms size as it is
}

int impnn_encoder_prepare_weights_gates(const float* weights, const float* bond_table, const float* atom_table,
                                        int32_t Va, int32_t D, int32_t K, int32_t S, int32_t Vb, int32_t mode,
                                        void* prepared, size_t prepared_bytes, impnn_stream_t stream) {
  REQUIRE(D > 0 && K > 0 && S >= 0 && Vb > 0 && Va > 0, "bad shape");
  REQUIRE(mode >= 0 && mode <= 3, "mode must be 0 (f32), 1 (f16x2), 2 (f32 typed) or 3 (f32x3 typed)");
  if (!encoder_fused_supported(mode, 1, 0, D, K, S, mode >= 2 ? Vb : 1))
    return fail(IMPNN_E_UNSUPPORTED, "encoder_prepare_weights_gates: mode=%d D=%d K=%d Vb=%d not covered", mode, D, K, Vb);
  if (S == 0) return IMPNN_OK;
  REQUIRE(weights && prepared && atom_table && (mode < 2 || bond_table), "null pointer");
  REQUIRE(aligned16(prepared) && aligned16(atom_table), "prepared buffer and atom_table must be 16B aligned");
  if (prepared_bytes < impnn_encoder_prepared_bytes_gates(D, S, Va, Vb, mode))
    return fail(IMPNN_E_WORKSPACE, "encoder_prepare_weights_gates: buffer %zu < %zu bytes", prepared_bytes,
                impnn_encoder_prepared_bytes_gates(D, S, Va, Vb, mode));
  return launch_encoder_prepare_gates(weights, bond_table, atom_table, Va, D, K, S, Vb, mode, prepared, as_stream(stream));
}

int impnn_encoder_fused_prepared(int32_t n_ions, const int32_t* const* atom_ids, const int32_t* const* bond_ids,
                                 const int32_t* const* conn, const float* atom_table, int32_t Va,
                                 const float* bond_table, int32_t Vb, const void* const* prepared, int32_t mode,
                                 float* const* pooled, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                                 int32_t S, float ln_eps, int32_t workgroups, void* workspace, size_t workspace_bytes,
                                 impnn_stream_t stream) {
  return encoder_common(__func__, n_ions, atom_ids, bond_ids, conn, atom_table, Va, bond_table, Vb, nullptr, prepared,
                        mode, pooled, B, N, E, D, K, S, ln_eps, workgroups, nullptr, nullptr, workspace,
                        workspace_bytes, stream);
}

int64_t impnn_model_head_floats(int32_t kind, int32_t D, int32_t F, int32_t Mx) {
  if (D <= 0 || F <= 0 || Mx <= 0 || (kind != 0 && kind != 1)) return -1;
  const int64_t common = 2 * ((int64_t)D * F + F) + 2 * ((int64_t)F * Mx + Mx);
  return common + (kind == 0 ? (int64_t)Mx * 3 + 3 : (int64_t)Mx * F + F + F + 1);
}

int impnn_model_head(int32_t kind, const float* pooled_cat, const float* pooled_an, const float* temperature,
                     const float* head_weights, float* out, int32_t B, int32_t D, int32_t F, int32_t Mx,
                     impnn_stream_t stream) {
  ModelHeadCall c = model_head(__func__, kind, pooled_cat, pooled_an, temperature, B, D, F, Mx, stream);
  c.w = head_weights, c.out = out;
  return model_head_checked(c, {true, head_weights && out, launch_model_head});
}

int impnn_model_head_tensors(int32_t kind, const float* pooled_cat, const float* pooled_an, const float* temperature,
                             const float* const* weights, float* out, int32_t B, int32_t D, int32_t F, int32_t Mx,
                             impnn_stream_t stream) {
  ModelHeadCall c = model_head(__func__, kind, pooled_cat, pooled_an, temperature, B, D, F, Mx, stream);
  c.weights = weights, c.out = out;
  return model_head_checked(c, {true, weights && out, launch_model_head_tensors});
}

int impnn_model_head_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an, const float* temperature,
                         const float* const* weights, const float* dout, float* dpooled_cat, float* dpooled_an,
                         float* const* dweights, int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  ModelHeadCall c = model_head(__func__, kind, pooled_cat, pooled_an, temperature, B, D, F, Mx, stream);
  c.weights = weights, c.dout = dout, c.dpc = dpooled_cat, c.dpa = dpooled_an, c.dweights = dweights;
  return model_head_checked(c, {true, weights && dout && dpooled_cat && dpooled_an && dweights, launch_model_head_bwd});
}

int64_t impnn_model_head_bwd_max_floats(void) { return model_head_bwd_max_floats(); }

int64_t impnn_model_head_loss_workspace_floats(int32_t B) { return B > 0 ? model_head_loss_workspace_floats(B) : 4; }

// The loss entries are the weighted launcher with a null weight: one body each, named for the entry that was called.
namespace {
int model_head_loss_entry(const char* entry, int32_t kind, const float* pooled_cat, const float* pooled_an,
                          const float* temperature, const float* const* weights, const float* l2, const float* y,
                          const float* sample_weight, float* pred, float* loss, float* workspace,
                          int64_t workspace_floats, int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  ModelHeadCall c = model_head(entry, kind, pooled_cat, pooled_an, temperature, B, D, F, Mx, stream);
  c.weights = weights, c.l2 = l2, c.y = y, c.sample_weight = sample_weight, c.out = pred, c.loss = loss;
  c.workspace = workspace, c.workspace_floats = workspace_floats;
  return model_head_checked(c, {false, weights && l2 && y && loss && workspace, launch_model_head_tensors});
}
int model_head_loss_bwd_entry(const char* entry, int32_t kind, const float* pooled_cat, const float* pooled_an,
                              const float* temperature, const float* const* weights, const float* l2, const float* y,
                              const float* sample_weight, const float* dloss, float* dpooled_cat, float* dpooled_an,
                              float* const* dweights, int32_t B, int32_t D, int32_t F, int32_t Mx,
                              impnn_stream_t stream) {
  ModelHeadCall c = model_head(entry, kind, pooled_cat, pooled_an, temperature, B, D, F, Mx, stream);
  c.weights = weights, c.l2 = l2, c.y = y, c.sample_weight = sample_weight, c.dloss = dloss, c.dpc = dpooled_cat;
  c.dpa = dpooled_an, c.dweights = dweights;
  return model_head_checked(c, {false, weights && l2 && y && dloss && dpooled_cat && dpooled_an && dweights,
                                launch_model_head_bwd});
}
}  // namespace

int impnn_model_head_loss(int32_t kind, const float* pooled_cat, const float* pooled_an, const float* temperature,
                          const float* const* weights, const float* l2, const float* y, float* pred, float* loss,
                          float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F, int32_t Mx,
                          impnn_stream_t stream) {
  return model_head_loss_entry(__func__, kind, pooled_cat, pooled_an, temperature, weights, l2, y, nullptr, pred, loss,
                               workspace, workspace_floats, B, D, F, Mx, stream);
}

int impnn_weighted_model_head_loss(int32_t kind, const float* pooled_cat, const float* pooled_an,
                                   const float* temperature, const float* const* weights, const float* l2,
                                   const float* y, const float* sample_weight, float* pred, float* loss,
                                   float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F,
                                   int32_t Mx, impnn_stream_t stream) {
  return model_head_loss_entry(__func__, kind, pooled_cat, pooled_an, temperature, weights, l2, y, sample_weight, pred,
                               loss, workspace, workspace_floats, B, D, F, Mx, stream);
}

int impnn_model_head_loss_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an, const float* temperature,
                              const float* const* weights, const float* l2, const float* y, const float* dloss,
                              float* dpooled_cat, float* dpooled_an, float* const* dweights, int32_t B, int32_t D,
                              int32_t F, int32_t Mx, impnn_stream_t stream) {
  return model_head_loss_bwd_entry(__func__, kind, pooled_cat, pooled_an, temperature, weights, l2, y, nullptr, dloss,
                                   dpooled_cat, dpooled_an, dweights, B, D, F, Mx, stream);
}

int impnn_weighted_model_head_loss_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an,
                                       const float* temperature, const float* const* weights, const float* l2,
                                       const float* y, const float* sample_weight, const float* dloss,
                                       float* dpooled_cat, float* dpooled_an, float* const* dweights, int32_t B,
                                       int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  return model_head_loss_bwd_entry(__func__, kind, pooled_cat, pooled_an, temperature, weights, l2, y, sample_weight,
                                   dloss, dpooled_cat, dpooled_an, dweights, B, D, F, Mx, stream);
}

// ---- the operands of a grid launch, as the C entries take them: the head form and the transfer form
namespace {
GridOperands head_grid_operands(int kind, const float* mix_cat, const float* mix_an, const float* T, const float* w, int C,
                                int A, int nT, int D, int F, int Mx, impnn_stream_t stream) {
  return {0, kind, mix_cat, mix_an, T, w, C, A, nT, D, F, Mx, as_stream(stream)};
}
GridOperands transfer_grid_operands(const float* u_cat, const float* u_an, const float* image, int C, int A,
                                    impnn_stream_t stream) {
  return {1, 1, u_cat, u_an, nullptr, image, C, A, 0, 0, 0, 0, as_stream(stream)};
}
// family 2: M members' mixing rows (M,C,Mx) / (M,A,Mx) and tails; no D
GridOperands ensemble_grid_operands(int kind, int M, const float* mix_cat, const float* mix_an, const float* T,
                                    const float* tails, float kappa, int C, int A, int nT, int F, int Mx,
                                    impnn_stream_t stream) {
  return {2, kind, mix_cat, mix_an, T, tails, C, A, nT, 0, F, Mx, as_stream(stream), M, kappa};
}
// family 3: the transfer grid's operands, S samples' multipliers (S,128) and kappa
GridOperands transfer_mc_grid_operands(const float* u_cat, const float* u_an, const float* image,
                                       const float* multipliers, int S, float kappa, int C, int A,
                                       impnn_stream_t stream) {
  return {3, 1, u_cat, u_an, nullptr, image, C, A, 0, 0, 0, 0, as_stream(stream), S, kappa, multipliers};
}
// the transfer grid's operands: 16-byte alignment, then the image size (image_floats < 0: the entry takes no image)
int transfer_image_rule(const char* entry, bool aligned_ok, int64_t image_floats) {
  if (!aligned_ok) return fail(IMPNN_E_BADARG, "%s: u rows and the image must be 16-byte aligned", entry);
  if (image_floats >= 0 && image_floats < transfer_grid_image_floats())
    return fail(IMPNN_E_WORKSPACE, "%s: image of %lld floats is too small (%lld)", entry, (long long)image_floats,
                (long long)transfer_grid_image_floats());
  return IMPNN_OK;
}
}  // namespace

// ---- the head over a cation x anion grid (include/impnn.h; head_grid.hip).  The family's order: shape, zero work,
// null pointers.
int impnn_head_ion_mix(int32_t kind, int32_t ion, const float* pooled, const float* head_weights, float* mix, int32_t M,
                       int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  REQUIRE(kind == 0 || kind == 1, "kind must be 0 (viscosity) or 1 (melting point)");
  REQUIRE(ion == 0 || ion == 1, "ion must be 0 (cation) or 1 (anion)");
  REQUIRE(M >= 0 && D > 0 && F > 0 && Mx > 0, "bad shape");
  if (int rc = head_widths_covered(__func__, D, F, Mx)) return rc;
  if (M == 0) return IMPNN_OK;
  REQUIRE(pooled && head_weights && mix, "null pointer");
  return launch_head_ion_mix(kind, ion, pooled, head_weights, mix, M, D, F, Mx, as_stream(stream));
}

int impnn_head_grid(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                    const float* head_weights, float* out, float* params, int32_t C, int32_t A, int32_t nT, int32_t D,
                    int32_t F, int32_t Mx, impnn_stream_t stream) {
  REQUIRE(kind == 0 || kind == 1, "kind must be 0 (viscosity) or 1 (melting point)");
  REQUIRE(C >= 0 && A >= 0 && nT >= 0 && D > 0 && F > 0 && Mx > 0, "bad shape");
  REQUIRE(kind == 1 || nT >= 1, "the viscosity grid needs nT >= 1 temperatures");
  REQUIRE(kind == 0 || nT == 0, "the melting-point grid takes no temperatures: nT must be 0");
  if (int rc = head_widths_covered(__func__, D, F, Mx)) return rc;
  if (nT > head_grid_max_temperatures())
    return fail(IMPNN_E_UNSUPPORTED, "%s: nT=%d temperatures (<= %d per call)", __func__, nT, head_grid_max_temperatures());
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(mix_cat && mix_an && head_weights && out && (kind == 1 || temperatures), "null pointer");
  REQUIRE(kind == 0 || (!temperatures && !params), "the melting-point grid takes neither temperatures nor params");
  return launch_head_grid(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                          out, params);
}

// ---- the transfer head (include/impnn.h; transfer_head.hip)
int64_t impnn_transfer_head_saved_floats(int32_t B, int32_t F, int32_t Mx) {
  return B > 0 && F > 0 && Mx > 0 ? transfer_head_saved_floats(B, F, Mx) : -1;
}
int64_t impnn_transfer_head_bwd_workspace_floats(int32_t B, int32_t F, int32_t Mx) {
  return B > 0 && F > 0 && Mx > 0 ? transfer_head_bwd_workspace_floats(B, F, Mx) : -1;
}
int64_t impnn_transfer_head_loss_workspace_floats(int32_t B) {
  return B > 0 ? transfer_head_loss_workspace_floats(B) : 4;
}

int impnn_transfer_head(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                        const float* moving_mean, const float* moving_var, float bn_eps, float* out, int32_t B,
                        int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  REQUIRE(B >= 0 && D > 0 && F > 0 && Mx > 0, "bad shape");
  REQUIRE(bn_eps >= 0.f, "bn_eps must not be negative");
  if (B == 0) return IMPNN_OK;
  REQUIRE(pooled_cat && pooled_an && weights && moving_mean && moving_var && out, "null pointer");
  TransferHeadCall c{};
  c.pc = pooled_cat, c.pa = pooled_an, c.weights = weights, c.bn_eps = bn_eps, c.out = out;
  c.moving_mean = const_cast<float*>(moving_mean), c.moving_var = const_cast<float*>(moving_var);  // read only here
  c.B = B, c.D = D, c.F = F, c.Mx = Mx, c.stream = as_stream(stream);
  return launch_transfer_head(c);
}

// The loss entries are the weighted launcher with a null weight (as the model head's): one body per direction, which
// names the entry that was called in its errors.  The *_rows entries are the same bodies with an index (ThRows): a
// null ThRows is the call as it was.
namespace {
struct ThRows {
  const int32_t *cat_row, *an_row;
  int32_t C, A;
};
#define REQUIRE_IN(entry, cond, what)                                 \
  do {                                                                \
    if (!(cond)) return fail(IMPNN_E_BADARG, "%s: %s", entry, what);  \
  } while (0)

// the index of an indexed entry, behind the null pointers and the weights' alignment
int check_th_rows(const char* entry, const ThRows& r) {
  REQUIRE_IN(entry, r.cat_row && r.an_row, "null row index");
  REQUIRE_IN(entry, reinterpret_cast<uintptr_t>(r.cat_row) % sizeof(int32_t) == 0 &&
                        reinterpret_cast<uintptr_t>(r.an_row) % sizeof(int32_t) == 0,
             "cat_row and an_row must be 4-byte aligned");
  REQUIRE_IN(entry, r.C >= 1 && r.A >= 1, "the tables need at least one row each (C, A >= 1)");
  return IMPNN_OK;
}

int transfer_head_loss_entry(const char* entry, const float* pooled_cat, const float* pooled_an,
                             const float* const* weights, const float* l2, float* moving_mean, float* moving_var,
                             float bn_momentum, float bn_eps, int32_t bn_batch, const float* y,
                             const float* sample_weight, int32_t loss_kind, float delta, float rate, uint64_t seed,
                             const int64_t* step, int32_t layer_word, float* saved, int64_t saved_floats, float* pred,
                             float* loss, float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F,
                             int32_t Mx, impnn_stream_t stream, const ThRows* rows = nullptr) {
  TransferHeadCall c{};
  c.dropout = rate != 0.f;
  if (c.dropout) {
    if (int rc = check_dropout(entry, rate, seed, step, layer_word, &c.drop)) return rc;
  }
  REQUIRE_IN(entry, (B > 0 || (rows && B == 0)) && D > 0 && F > 0 && Mx > 0, "bad shape");
  if (B == 0) return IMPNN_OK;  // (an indexed entry only: no sample, nothing is touched)
  REQUIRE_IN(entry, loss_kind == 0 || (loss_kind == 1 && delta > 0.f),
             "loss_kind must be 0 (squared error) or 1 (Huber, delta > 0)");
  REQUIRE_IN(entry, bn_eps >= 0.f && bn_momentum >= 0.f && bn_momentum <= 1.f,
             "bn_eps >= 0 and 0 <= bn_momentum <= 1 required");
  REQUIRE_IN(entry, pooled_cat && pooled_an && weights && l2 && moving_mean && moving_var && y && loss && workspace,
             "null pointer");
  REQUIRE_IN(entry, reinterpret_cast<uintptr_t>(sample_weight) % sizeof(float) == 0,
             "sample_weight must be 4-byte aligned");
  if (rows) {
    if (int rc = check_th_rows(entry, *rows)) return rc;
    c.cat_row = rows->cat_row, c.an_row = rows->an_row, c.C = rows->C, c.A = rows->A;
  }
  REQUIRE_IN(entry, saved || !bn_batch, "the batch statistics need the saved buffer");
  if (saved && saved_floats < transfer_head_saved_floats(B, F, Mx))
    return fail(IMPNN_E_WORKSPACE, "%s: saved buffer of %lld floats is too small", entry, (long long)saved_floats);
  if (workspace_floats < impnn_transfer_head_loss_workspace_floats(B))
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %lld floats is too small", entry, (long long)workspace_floats);
  c.pc = pooled_cat, c.pa = pooled_an, c.weights = weights, c.l2 = l2, c.moving_mean = moving_mean;
  c.moving_var = moving_var, c.bn_momentum = bn_momentum, c.bn_eps = bn_eps, c.bn_batch = bn_batch != 0, c.y = y;
  c.sample_weight = sample_weight;
  c.loss_kind = loss_kind, c.delta = delta, c.saved = saved, c.out = pred, c.loss = loss, c.workspace = workspace;
  c.B = B, c.D = D, c.F = F, c.Mx = Mx, c.stream = as_stream(stream);
  return launch_transfer_head(c);
}

int transfer_head_loss_bwd_entry(const char* entry, const float* pooled_cat, const float* pooled_an,
                                 const float* const* weights, float* const* dweights, const float* l2,
                                 int32_t bn_batch, const float* y, const float* sample_weight, int32_t loss_kind,
                                 float delta, const float* dloss, float rate, uint64_t seed, const int64_t* step,
                                 int32_t layer_word, const float* saved, int64_t saved_floats, float* workspace,
                                 int64_t workspace_floats, float* dpooled_cat, float* dpooled_an, int32_t B, int32_t D,
                                 int32_t F, int32_t Mx, impnn_stream_t stream, const ThRows* rows = nullptr) {
  TransferHeadCall c{};
  c.dropout = rate != 0.f;
  if (c.dropout) {
    if (int rc = check_dropout(entry, rate, seed, step, layer_word, &c.drop)) return rc;
  }
  REQUIRE_IN(entry, (B > 0 || (rows && B == 0)) && D > 0 && F > 0 && Mx > 0, "bad shape");
  if (B == 0) return IMPNN_OK;  // (an indexed entry only: no sample, no gradient is added)
  REQUIRE_IN(entry, loss_kind == 0 || (loss_kind == 1 && delta > 0.f),
             "loss_kind must be 0 (squared error) or 1 (Huber, delta > 0)");
  REQUIRE_IN(entry, pooled_cat && pooled_an && weights && dweights && l2 && y && dloss && saved && workspace,
             "null pointer");
  REQUIRE_IN(entry, reinterpret_cast<uintptr_t>(sample_weight) % sizeof(float) == 0,
             "sample_weight must be 4-byte aligned");
  if (rows) {
    if (int rc = check_th_rows(entry, *rows)) return rc;
    c.cat_row = rows->cat_row, c.an_row = rows->an_row, c.C = rows->C, c.A = rows->A;
  }
  REQUIRE_IN(entry, (dpooled_cat != nullptr) == (dpooled_an != nullptr), "dpooled_cat and dpooled_an: both or neither");
  if (saved_floats < transfer_head_saved_floats(B, F, Mx))
    return fail(IMPNN_E_WORKSPACE, "%s: saved buffer of %lld floats is too small", entry, (long long)saved_floats);
  if (workspace_floats < transfer_head_bwd_workspace_floats(B, F, Mx))
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %lld floats is too small", entry, (long long)workspace_floats);
  c.pc = pooled_cat, c.pa = pooled_an, c.weights = weights, c.dweights = dweights, c.l2 = l2;
  c.bn_batch = bn_batch != 0, c.y = y, c.sample_weight = sample_weight, c.loss_kind = loss_kind, c.delta = delta;
  c.dloss = dloss;
  c.saved = const_cast<float*>(saved), c.workspace = workspace, c.dpc = dpooled_cat, c.dpa = dpooled_an;
  c.B = B, c.D = D, c.F = F, c.Mx = Mx, c.stream = as_stream(stream);
  return launch_transfer_head_bwd(c);
}
#undef REQUIRE_IN
}  // namespace

int impnn_transfer_head_loss(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                             const float* l2, float* moving_mean, float* moving_var, float bn_momentum, float bn_eps,
                             int32_t bn_batch, const float* y, int32_t loss_kind, float delta, float rate,
                             uint64_t seed, const int64_t* step, int32_t layer_word, float* saved,
                             int64_t saved_floats, float* pred, float* loss, float* workspace,
                             int64_t workspace_floats, int32_t B, int32_t D, int32_t F, int32_t Mx,
                             impnn_stream_t stream) {
  return transfer_head_loss_entry(__func__, pooled_cat, pooled_an, weights, l2, moving_mean, moving_var, bn_momentum,
                                  bn_eps, bn_batch, y, nullptr, loss_kind, delta, rate, seed, step, layer_word, saved,
                                  saved_floats, pred, loss, workspace, workspace_floats, B, D, F, Mx, stream);
}

int impnn_weighted_transfer_head_loss(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                      const float* l2, float* moving_mean, float* moving_var, float bn_momentum,
                                      float bn_eps, int32_t bn_batch, const float* y, const float* sample_weight,
                                      int32_t loss_kind, float delta, float rate, uint64_t seed, const int64_t* step,
                                      int32_t layer_word, float* saved, int64_t saved_floats, float* pred, float* loss,
                                      float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F,
                                      int32_t Mx, impnn_stream_t stream) {
  return transfer_head_loss_entry(__func__, pooled_cat, pooled_an, weights, l2, moving_mean, moving_var, bn_momentum,
                                  bn_eps, bn_batch, y, sample_weight, loss_kind, delta, rate, seed, step, layer_word,
                                  saved, saved_floats, pred, loss, workspace, workspace_floats, B, D, F, Mx, stream);
}

int impnn_transfer_head_loss_bwd(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                 float* const* dweights, const float* l2, int32_t bn_batch, const float* y,
                                 int32_t loss_kind, float delta, const float* dloss, float rate, uint64_t seed,
                                 const int64_t* step, int32_t layer_word, const float* saved, int64_t saved_floats,
                                 float* workspace, int64_t workspace_floats, float* dpooled_cat, float* dpooled_an,
                                 int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  return transfer_head_loss_bwd_entry(__func__, pooled_cat, pooled_an, weights, dweights, l2, bn_batch, y, nullptr,
                                      loss_kind, delta, dloss, rate, seed, step, layer_word, saved, saved_floats,
                                      workspace, workspace_floats, dpooled_cat, dpooled_an, B, D, F, Mx, stream);
}

int impnn_weighted_transfer_head_loss_bwd(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                          float* const* dweights, const float* l2, int32_t bn_batch, const float* y,
                                          const float* sample_weight, int32_t loss_kind, float delta,
                                          const float* dloss, float rate, uint64_t seed, const int64_t* step,
                                          int32_t layer_word, const float* saved, int64_t saved_floats,
                                          float* workspace, int64_t workspace_floats, float* dpooled_cat,
                                          float* dpooled_an, int32_t B, int32_t D, int32_t F, int32_t Mx,
                                          impnn_stream_t stream) {
  return transfer_head_loss_bwd_entry(__func__, pooled_cat, pooled_an, weights, dweights, l2, bn_batch, y,
                                      sample_weight, loss_kind, delta, dloss, rate, seed, step, layer_word, saved,
                                      saved_floats, workspace, workspace_floats, dpooled_cat, dpooled_an, B, D, F, Mx,
                                      stream);
}

int impnn_transfer_head_loss_rows(const float* cat_table, const float* an_table, const int32_t* cat_row,
                                  const int32_t* an_row, const float* const* weights, const float* l2,
                                  float* moving_mean, float* moving_var, float bn_momentum, float bn_eps,
                                  int32_t bn_batch, const float* y, const float* sample_weight, int32_t loss_kind,
                                  float delta, float rate, uint64_t seed, const int64_t* step, int32_t layer_word,
                                  float* saved, int64_t saved_floats, float* pred, float* loss, float* workspace,
                                  int64_t workspace_floats, int32_t B, int32_t C, int32_t A, int32_t D, int32_t F,
                                  int32_t Mx, impnn_stream_t stream) {
  const ThRows rows{cat_row, an_row, C, A};
  return transfer_head_loss_entry(__func__, cat_table, an_table, weights, l2, moving_mean, moving_var, bn_momentum,
                                  bn_eps, bn_batch, y, sample_weight, loss_kind, delta, rate, seed, step, layer_word,
                                  saved, saved_floats, pred, loss, workspace, workspace_floats, B, D, F, Mx, stream,
                                  &rows);
}

int impnn_transfer_head_loss_rows_bwd(const float* cat_table, const float* an_table, const int32_t* cat_row,
                                      const int32_t* an_row, const float* const* weights, float* const* dweights,
                                      const float* l2, int32_t bn_batch, const float* y, const float* sample_weight,
                                      int32_t loss_kind, float delta, const float* dloss, float rate, uint64_t seed,
                                      const int64_t* step, int32_t layer_word, const float* saved,
                                      int64_t saved_floats, float* workspace, int64_t workspace_floats, int32_t B,
                                      int32_t C, int32_t A, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  const ThRows rows{cat_row, an_row, C, A};
  return transfer_head_loss_bwd_entry(__func__, cat_table, an_table, weights, dweights, l2, bn_batch, y,
                                      sample_weight, loss_kind, delta, dloss, rate, seed, step, layer_word, saved,
                                      saved_floats, workspace, workspace_floats, nullptr, nullptr, B, D, F, Mx, stream,
                                      &rows);
}

// ---- the transfer head over a cation x anion grid (include/impnn.h; transfer_grid.hip).  One place applies the
// family's rules in their fixed order: shape, zero work, null pointers (then alignment and the image size), ranges.
namespace {
struct TransferGridCheck {
  const char* entry;
  bool shape_ok;
  bool zero_work;
  bool pointers_ok;
  bool weights_needed;            // the 18-pointer table is read
  const float* const* weights;
  bool aligned_ok;
  int64_t image_floats;           // < 0: the entry takes no image
  int D, F, Mx;                   // D == 0: the entry takes no widths
};
// IMPNN_OK with *launch == false: success with nothing to do
int transfer_grid_check(const TransferGridCheck& c, bool* launch) {
  *launch = false;
  if (!c.shape_ok) return fail(IMPNN_E_BADARG, "%s: bad shape", c.entry);
  if (c.zero_work) return IMPNN_OK;
  if (!c.pointers_ok) return fail(IMPNN_E_BADARG, "%s: null pointer", c.entry);
  if (c.weights_needed)
    for (int t = 0; t < kThTensors; ++t)
      if (!c.weights[t]) return fail(IMPNN_E_BADARG, "%s: null weight tensor %d", c.entry, t);
  if (int rc = transfer_image_rule(c.entry, c.aligned_ok, c.image_floats)) return rc;
  if (int rc = head_widths_covered(c.entry, c.D, c.F, c.Mx)) return rc;
  *launch = true;
  return IMPNN_OK;
}
}  // namespace

int64_t impnn_transfer_grid_image_floats(void) { return transfer_grid_image_floats(); }

int impnn_transfer_grid_prepare(const float* const* weights, const float* moving_mean, const float* moving_var,
                                float bn_eps, float* image, int64_t image_floats, impnn_stream_t stream) {
  TransferGridCheck c{};
  c.entry = __func__, c.shape_ok = bn_eps >= 0.f && image_floats >= 0;
  c.pointers_ok = weights && moving_mean && moving_var && image;
  c.weights_needed = true, c.weights = weights, c.aligned_ok = aligned16(image), c.image_floats = image_floats;
  bool launch;
  if (int rc = transfer_grid_check(c, &launch)) return rc;
  return launch ? launch_transfer_grid_prepare(weights, moving_mean, moving_var, bn_eps, image, as_stream(stream)) : IMPNN_OK;
}

int impnn_transfer_ion_half(int32_t ion, const float* pooled, const float* const* weights, float* u, int32_t M,
                            int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  TransferGridCheck c{};
  c.entry = __func__, c.shape_ok = (ion == 0 || ion == 1) && M >= 0 && D > 0 && F > 0 && Mx > 0;
  c.zero_work = M == 0, c.pointers_ok = pooled && weights && u;
  c.weights_needed = true, c.weights = weights, c.aligned_ok = true, c.image_floats = -1;
  c.D = D, c.F = F, c.Mx = Mx;
  bool launch;
  if (int rc = transfer_grid_check(c, &launch)) return rc;
  return launch ? launch_transfer_ion_half(ion, pooled, weights, u, M, D, F, Mx, as_stream(stream)) : IMPNN_OK;
}

int impnn_transfer_head_grid(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                             float* out, int32_t C, int32_t A, impnn_stream_t stream) {
  TransferGridCheck c{};
  c.entry = __func__, c.shape_ok = C >= 0 && A >= 0 && image_floats >= 0;
  c.zero_work = C == 0 || A == 0, c.pointers_ok = u_cat && u_an && image && out;
  c.aligned_ok = aligned16(u_cat) && aligned16(u_an) && aligned16(image), c.image_floats = image_floats;
  bool launch;
  if (int rc = transfer_grid_check(c, &launch)) return rc;
  return launch ? launch_transfer_head_grid(transfer_grid_operands(u_cat, u_an, image, C, A, stream), out) : IMPNN_OK;
}

// ---- the screening family over a cation x anion grid: top-k (grid_select.hip), best partners (grid_partners.hip), the
// rank cut (grid_rank.hip), pair masks (grid_mask.hip).  Each rule the entries share is one helper that takes the
// entry's name; each *_checked below lists them in its own fixed order (tests/test_cabi.py and the host tests pin it).
namespace {
int grid_family_rule(const char* entry, int family) {
  if (family != 0 && family != 1) return fail(IMPNN_E_BADARG, "%s: family must be 0 (head grid) or 1 (transfer grid)", entry);
  return IMPNN_OK;
}
// the kind, the entry's signs (`shape_ok`), then the temperature count the kind allows (a negative nT is a bad shape)
int grid_kind_rule(const char* entry, const GridOperands& g, bool shape_ok) {
  if (g.family != 1 && g.kind != 0 && g.kind != 1)
    return fail(IMPNN_E_BADARG, "%s: kind must be 0 (viscosity) or 1 (melting point)", entry);
  if (!shape_ok) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (g.family != 1 && g.kind == 0 && g.nT == 0) return fail(IMPNN_E_BADARG, "%s: the viscosity grid needs nT >= 1 temperatures", entry);
  if (g.family != 1 && g.kind == 1 && g.nT > 0)
    return fail(IMPNN_E_BADARG, "%s: the melting-point grid takes no temperatures: nT must be 0", entry);
  return IMPNN_OK;
}
int grid_no_temperatures_rule(const char* entry, const GridOperands& g) {
  if (g.family != 1 && g.kind == 1 && g.T) return fail(IMPNN_E_BADARG, "%s: the melting-point grid takes no temperatures", entry);
  return IMPNN_OK;
}
// the families whose operands are u rows and the prepared image: no widths, no temperatures
bool grid_takes_image(const GridOperands& g) { return g.family == 1 || g.family == 3; }
int grid_transfer_rule(const char* entry, const GridOperands& g, int64_t image_floats) {
  if (!grid_takes_image(g)) return IMPNN_OK;
  if (int rc = transfer_image_rule(entry, aligned16(g.mix_cat) && aligned16(g.mix_an) && aligned16(g.w), image_floats))
    return rc;
  if (g.family == 3 && !aligned16(g.multipliers))
    return fail(IMPNN_E_BADARG, "%s: the multipliers must be 16-byte aligned", entry);
  return IMPNN_OK;
}
// workspace alignment (8 bytes) and mask alignment (4): `message` names the entry's buffers; q may be null
int grid_aligned_rule(const char* entry, const void* p, const void* q, unsigned bytes, const char* message) {
  if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & (bytes - 1)) != 0)
    return fail(IMPNN_E_BADARG, "%s: %s", entry, message);
  return IMPNN_OK;
}
int grid_workspace_rule(const char* entry, size_t workspace_bytes, size_t need) {
  if (workspace_bytes < need)
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %zu bytes is too small (%zu)", entry, workspace_bytes, need);
  return IMPNN_OK;
}
int grid_select_temperatures_rule(const char* entry, int nT, int most = kSelectMaxT) {
  if (nT > most)
    return fail(IMPNN_E_UNSUPPORTED, "%s: nT=%d temperatures (<= %d per selecting call)", entry, nT, most);
  return IMPNN_OK;
}
// the ensemble's own arguments, checked with the shape (a head or transfer grid has none)
int grid_ensemble_rule(const char* entry, int M, float kappa) {
  if (M < 1) return fail(IMPNN_E_BADARG, "%s: M=%d members must be at least 1", entry, M);
  if (M > ensemble_grid_max_members())
    return fail(IMPNN_E_UNSUPPORTED, "%s: M=%d members (<= %d per call)", entry, M, ensemble_grid_max_members());
  if (!(kappa - kappa == 0.f)) return fail(IMPNN_E_BADARG, "%s: kappa must be finite", entry);
  return IMPNN_OK;
}
// the transfer MC grid's own arguments, checked with the shape
int grid_mc_rule(const char* entry, int S, float kappa) {
  if (S < 1) return fail(IMPNN_E_BADARG, "%s: S=%d samples must be at least 1", entry, S);
  if (S > transfer_mc_grid_max_samples())
    return fail(IMPNN_E_UNSUPPORTED, "%s: S=%d samples (<= %d per call)", entry, S, transfer_mc_grid_max_samples());
  if (!(kappa - kappa == 0.f)) return fail(IMPNN_E_BADARG, "%s: kappa must be finite", entry);
  return IMPNN_OK;
}
int grid_pairs_rule(const char* entry, int C, int A) {
  if ((int64_t)C * A >= (int64_t)1 << 32)
    return fail(IMPNN_E_UNSUPPORTED, "%s: %lld pairs (< 2^32 per call); split the cation axis", entry,
                (long long)((int64_t)C * A));
  return IMPNN_OK;
}

// shape only: what the workspace query and the entries share
int grid_topk_limits(const char* entry, int C, int A, int nT, int k, int workgroups, int most_temperatures) {
  if (C < 0 || A < 0 || nT < 0 || workgroups < 0) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (k < 1) return fail(IMPNN_E_BADARG, "%s: k=%d must be at least 1", entry, k);
  if (k > kSelectMaxK) return fail(IMPNN_E_UNSUPPORTED, "%s: k=%d entries (<= %d per call)", entry, k, kSelectMaxK);
  if (int rc = grid_select_temperatures_rule(entry, nT, most_temperatures)) return rc;
  return grid_pairs_rule(entry, C, A);
}
int grid_topk_shape(const char* entry, int family, int C, int A, int nT, int k, int workgroups) {
  if (int rc = grid_family_rule(entry, family)) return rc;
  return grid_topk_limits(entry, C, A, nT, k, workgroups, kSelectMaxT);
}
// the ensemble grid's: M and kappa first, then the same limits with the temperatures M members leave room for
int ensemble_topk_shape(const char* entry, int M, float kappa, int C, int A, int nT, int k, int workgroups) {
  if (int rc = grid_ensemble_rule(entry, M, kappa)) return rc;
  return grid_topk_limits(entry, C, A, nT, k, workgroups, ensemble_grid_topk_max_temperatures(M));
}
// the transfer MC grid's: S and kappa first, then the same limits (it takes no temperatures)
int mc_topk_shape(const char* entry, int S, float kappa, int C, int A, int k, int workgroups) {
  if (int rc = grid_mc_rule(entry, S, kappa)) return rc;
  return grid_topk_limits(entry, C, A, 0, k, workgroups, kSelectMaxT);
}
int grid_partners_shape(const char* entry, int family, int C, int A, int nT, int m) {
  if (int rc = grid_family_rule(entry, family)) return rc;
  if (C < 0 || A < 0 || nT < 0) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (m < 1) return fail(IMPNN_E_BADARG, "%s: m=%d must be at least 1", entry, m);
  if (m > kPartnersMaxM) return fail(IMPNN_E_UNSUPPORTED, "%s: m=%d partners (<= %d per call)", entry, m, kPartnersMaxM);
  if (int rc = grid_select_temperatures_rule(entry, nT)) return rc;
  return grid_pairs_rule(entry, C, A);
}
int grid_rank_limits(const char* entry, int C, int A, int nT) {
  if ((int64_t)C * A > kRankMaxPairs)
    return fail(IMPNN_E_UNSUPPORTED, "%s: %lld pairs (<= 2^32 - 2 per call)", entry, (long long)((int64_t)C * A));
  return grid_select_temperatures_rule(entry, nT);
}

// Top-k and best partners, after the entry's own shape rule: the widths' limits, zero work (IMPNN_OK with *launch ==
// false), null pointers, alignment and the image size, the workspace size (`need`: the entry's query for the shape).
int grid_selecting_rules(const char* entry, const GridOperands& g, bool pointers_ok, const void* workspace,
                         const uint32_t* where, int64_t image_floats, size_t need, size_t workspace_bytes, bool* launch) {
  *launch = false;
  if (!grid_takes_image(g))
    if (int rc = head_widths_covered(entry, g.D, g.F, g.Mx)) return rc;
  if (g.C == 0 || g.A == 0) return IMPNN_OK;
  if (!pointers_ok) return fail(IMPNN_E_BADARG, "%s: null pointer", entry);
  if (int rc = grid_no_temperatures_rule(entry, g)) return rc;
  if (int rc = grid_aligned_rule(entry, workspace, nullptr, 8, "the workspace must be 8-byte aligned")) return rc;
  if (int rc = grid_aligned_rule(entry, where, nullptr, 4, "the mask must be 4-byte aligned")) return rc;
  if (int rc = grid_transfer_rule(entry, g, image_floats)) return rc;
  if (int rc = grid_workspace_rule(entry, workspace_bytes, need)) return rc;
  *launch = true;
  return IMPNN_OK;
}

// shape_ok: the widths' signs (head grid), image_floats >= 0 (transfer grid)
int grid_topk_checked(const char* entry, const GridTopkCall& c, bool shape_ok, bool pointers_ok, int64_t image_floats,
                      size_t workspace_bytes) {
  const GridOperands& g = c.g;
  if (int rc = grid_kind_rule(entry, g, shape_ok)) return rc;
  if (int rc = g.family == 2   ? ensemble_topk_shape(entry, g.M, g.kappa, g.C, g.A, g.nT, c.k, c.workgroups)
               : g.family == 3 ? mc_topk_shape(entry, g.M, g.kappa, g.C, g.A, c.k, c.workgroups)
                               : grid_topk_shape(entry, g.family, g.C, g.A, g.nT, c.k, c.workgroups))
    return rc;
  bool launch;
  if (int rc = grid_selecting_rules(entry, g, pointers_ok && (!c.masked || c.where), c.workspace, c.where, image_floats,
                                    grid_topk_workspace_bytes(g.family, g.C, g.A, g.nT, c.k, c.workgroups), workspace_bytes,
                                    &launch))
    return rc;
  if (!launch) return IMPNN_OK;
  return g.family == 2 ? launch_ensemble_grid_topk(c) : g.family == 3 ? launch_transfer_mc_grid_topk(c) : launch_grid_topk(c);
}

int grid_partners_checked(const char* entry, const GridPartnersCall& c, bool shape_ok, bool pointers_ok,
                          int64_t image_floats, size_t workspace_bytes) {
  const GridOperands& g = c.g;
  if (int rc = grid_kind_rule(entry, g, shape_ok)) return rc;
  if (int rc = grid_partners_shape(entry, g.family, g.C, g.A, g.nT, c.m)) return rc;
  bool launch;
  if (int rc = grid_selecting_rules(entry, g, pointers_ok, c.workspace, c.where, image_floats,
                                    grid_partners_workspace_bytes(g.family, g.C, g.A, g.nT, c.m), workspace_bytes, &launch))
    return rc;
  return launch ? launch_grid_partners(c) : IMPNN_OK;
}

// The rank cut's order: kind, shape, zero work, null pointers (then alignment and the image size), k < 1, the
// pair-count limit, the nT limit, the workspace size, the widths.  Nothing is launched before the last.
int grid_rank_checked(const char* entry, const GridRankCall& c, bool shape_ok, bool pointers_ok, int64_t image_floats,
                      size_t workspace_bytes) {
  const GridOperands& g = c.g;
  if (int rc = grid_kind_rule(entry, g, shape_ok)) return rc;
  if (g.C < 0 || g.A < 0 || g.nT < 0 || c.workgroups < 0) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (g.C == 0 || g.A == 0) return IMPNN_OK;
  if (!pointers_ok) return fail(IMPNN_E_BADARG, "%s: null pointer", entry);
  if (int rc = grid_no_temperatures_rule(entry, g)) return rc;
  if (int rc = grid_aligned_rule(entry, c.workspace, c.count, 8, "the workspace and the counts must be 8-byte aligned")) return rc;
  if (int rc = grid_aligned_rule(entry, c.where, c.mask_words, 4, "the masks must be 4-byte aligned")) return rc;
  if (int rc = grid_transfer_rule(entry, g, image_floats)) return rc;
  if (c.k < 1) return fail(IMPNN_E_BADARG, "%s: k=%lld must be at least 1", entry, (long long)c.k);
  if (int rc = grid_rank_limits(entry, g.C, g.A, g.nT)) return rc;
  if (int rc = grid_workspace_rule(entry, workspace_bytes, grid_rank_workspace_bytes(g.family, g.C, g.A, g.nT, c.workgroups)))
    return rc;
  if (g.family == 0)
    if (int rc = head_widths_covered(entry, g.D, g.F, g.Mx)) return rc;
  return launch_grid_rank(c);
}

// The pair masks' order: kind, shape, the temperature count, a NaN bound, zero work, null pointers, alignment and the
// image size, the limits of one launch.
int grid_mask_checked(const char* entry, const GridMaskCall& c, bool shape_ok, bool pointers_ok, int64_t image_floats) {
  const GridOperands& g = c.g;
  if (int rc = grid_kind_rule(entry, g, shape_ok && g.C >= 0 && g.A >= 0 && g.nT >= 0)) return rc;
  if (g.family == 2)
    if (int rc = grid_ensemble_rule(entry, g.M, g.kappa)) return rc;
  if (g.family == 3)
    if (int rc = grid_mc_rule(entry, g.M, g.kappa)) return rc;
  if (c.lo != c.lo || c.hi != c.hi) return fail(IMPNN_E_BADARG, "%s: a bound is NaN (an infinity means no limit)", entry);
  if (g.C == 0 || g.A == 0) return IMPNN_OK;
  if (!pointers_ok) return fail(IMPNN_E_BADARG, "%s: null pointer", entry);
  if (int rc = grid_no_temperatures_rule(entry, g)) return rc;
  if (int rc = grid_aligned_rule(entry, c.words, nullptr, 4, "the mask must be 4-byte aligned")) return rc;
  if (int rc = grid_transfer_rule(entry, g, image_floats)) return rc;
  if (!grid_takes_image(g)) {
    if (int rc = head_widths_covered(entry, g.D, g.F, g.Mx)) return rc;
    const int most = g.family == 2 ? ensemble_grid_max_temperatures(g.kind, g.M) : head_grid_max_temperatures();
    if (g.nT > most) return fail(IMPNN_E_UNSUPPORTED, "%s: nT=%d temperatures (<= %d per call)", entry, g.nT, most);
  }
  return g.family == 2 ? launch_ensemble_grid_mask(c) : g.family == 3 ? launch_transfer_mc_grid_mask(c) : launch_grid_mask(c);
}
}  // namespace

int32_t impnn_grid_topk_max_temperatures(void) { return kSelectMaxT; }

int impnn_grid_topk_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t k, int32_t workgroups,
                                    size_t* need) {
  if (int rc = grid_topk_shape(__func__, family, C, A, nT, k, workgroups)) return rc;
  REQUIRE(need, "null pointer");
  *need = grid_topk_workspace_bytes(family, C, A, nT, k, workgroups);
  return IMPNN_OK;
}

int impnn_head_grid_topk(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, int32_t k, int32_t largest, float* values, int32_t* cation,
                         int32_t* anion, void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT,
                         int32_t D, int32_t F, int32_t Mx, int32_t workgroups, impnn_stream_t stream) {
  const GridTopkCall c{head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                       k, largest, values, cation, anion, workspace, workgroups, false, nullptr};
  return grid_topk_checked(__func__, c, D > 0 && F > 0 && Mx > 0,
                           mix_cat && mix_an && head_weights && values && cation && anion && workspace &&
                               (kind == 1 || temperatures),
                           0, workspace_bytes);
}

int impnn_transfer_head_grid_topk(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                  void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups,
                                  impnn_stream_t stream) {
  const GridTopkCall c{transfer_grid_operands(u_cat, u_an, image, C, A, stream), k, largest, values, cation, anion,
                       workspace, workgroups, false, nullptr};
  return grid_topk_checked(__func__, c, image_floats >= 0, u_cat && u_an && image && values && cation && anion && workspace,
                           image_floats, workspace_bytes);
}

int impnn_head_grid_topk_where(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                               const float* head_weights, const uint32_t* where, int32_t k, int32_t largest,
                               float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                               int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F, int32_t Mx, int32_t workgroups,
                               impnn_stream_t stream) {
  const GridTopkCall c{head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                       k, largest, values, cation, anion, workspace, workgroups, true, where};
  return grid_topk_checked(__func__, c, D > 0 && F > 0 && Mx > 0,
                           mix_cat && mix_an && head_weights && values && cation && anion && workspace &&
                               (kind == 1 || temperatures),
                           0, workspace_bytes);
}

int impnn_transfer_head_grid_topk_where(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                        const uint32_t* where, int32_t k, int32_t largest, float* values,
                                        int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                                        int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream) {
  const GridTopkCall c{transfer_grid_operands(u_cat, u_an, image, C, A, stream), k, largest, values, cation, anion,
                       workspace, workgroups, true, where};
  return grid_topk_checked(__func__, c, image_floats >= 0, u_cat && u_an && image && values && cation && anion && workspace,
                           image_floats, workspace_bytes);
}

int impnn_grid_partners_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t m, size_t* need) {
  if (int rc = grid_partners_shape(__func__, family, C, A, nT, m)) return rc;
  REQUIRE(need, "null pointer");
  *need = grid_partners_workspace_bytes(family, C, A, nT, m);
  return IMPNN_OK;
}

int impnn_head_grid_partners(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                             const float* head_weights, const uint32_t* where, int32_t m, int32_t largest,
                             float* cat_values, int32_t* cat_partner, float* an_values, int32_t* an_partner,
                             void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t D,
                             int32_t F, int32_t Mx, impnn_stream_t stream) {
  const GridPartnersCall c{head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                           where, m, largest, cat_values, cat_partner, an_values, an_partner, workspace};
  return grid_partners_checked(__func__, c, D > 0 && F > 0 && Mx > 0,
                               mix_cat && mix_an && head_weights && cat_values && cat_partner && an_values && an_partner &&
                                   workspace && (kind == 1 || temperatures),
                               0, workspace_bytes);
}

int impnn_transfer_head_grid_partners(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                      const uint32_t* where, int32_t m, int32_t largest, float* cat_values,
                                      int32_t* cat_partner, float* an_values, int32_t* an_partner, void* workspace,
                                      size_t workspace_bytes, int32_t C, int32_t A, impnn_stream_t stream) {
  const GridPartnersCall c{transfer_grid_operands(u_cat, u_an, image, C, A, stream), where, m, largest, cat_values,
                           cat_partner, an_values, an_partner, workspace};
  return grid_partners_checked(__func__, c, image_floats >= 0,
                               u_cat && u_an && image && cat_values && cat_partner && an_values && an_partner && workspace,
                               image_floats, workspace_bytes);
}

int32_t impnn_grid_rank_digit_bits(void) { return kRankDigitBits; }

int32_t impnn_grid_rank_passes(int32_t C, int32_t A) { return C < 0 || A < 0 ? 0 : grid_rank_passes((int64_t)C * A); }

int impnn_grid_rank_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t workgroups, size_t* need) {
  if (int rc = grid_family_rule(__func__, family)) return rc;
  if (C < 0 || A < 0 || nT < 0 || workgroups < 0) return fail(IMPNN_E_BADARG, "%s: bad shape", __func__);
  REQUIRE(need, "null pointer");
  if (int rc = grid_rank_limits(__func__, C, A, nT)) return rc;
  *need = grid_rank_workspace_bytes(family, C, A, nT, workgroups);
  return IMPNN_OK;
}

int impnn_head_grid_rank(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, int64_t k, int32_t largest, const uint32_t* where, float* values,
                         int32_t* cation, int32_t* anion, int64_t* count, uint32_t* mask_words, void* workspace,
                         size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F, int32_t Mx,
                         int32_t workgroups, impnn_stream_t stream) {
  const GridRankCall c{head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                       k, largest, where, values, cation, anion, count, mask_words, workspace, workgroups};
  return grid_rank_checked(__func__, c, D > 0 && F > 0 && Mx > 0,
                           mix_cat && mix_an && head_weights && values && cation && anion && count && workspace &&
                               (kind == 1 || temperatures),
                           0, workspace_bytes);
}

int impnn_transfer_head_grid_rank(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  int64_t k, int32_t largest, const uint32_t* where, float* values, int32_t* cation,
                                  int32_t* anion, int64_t* count, uint32_t* mask_words, void* workspace,
                                  size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream) {
  const GridRankCall c{transfer_grid_operands(u_cat, u_an, image, C, A, stream), k, largest, where, values, cation, anion,
                       count, mask_words, workspace, workgroups};
  return grid_rank_checked(__func__, c, image_floats >= 0,
                           u_cat && u_an && image && values && cation && anion && count && workspace, image_floats,
                           workspace_bytes);
}

int64_t impnn_grid_mask_row_words(int32_t A) { return grid_mask_row_words(A); }

int impnn_head_grid_mask(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, float lo, float hi, uint32_t* words, int32_t C, int32_t A,
                         int32_t nT, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream) {
  const GridMaskCall c{head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                       lo, hi, words};
  return grid_mask_checked(__func__, c, D > 0 && F > 0 && Mx > 0,
                           mix_cat && mix_an && head_weights && words && (kind == 1 || temperatures), 0);
}

int impnn_transfer_head_grid_mask(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  float lo, float hi, uint32_t* words, int32_t C, int32_t A, impnn_stream_t stream) {
  const GridMaskCall c{transfer_grid_operands(u_cat, u_an, image, C, A, stream), lo, hi, words};
  return grid_mask_checked(__func__, c, image_floats >= 0, u_cat && u_an && image && words, image_floats);
}

// ---- the ensemble grid (include/impnn.h; ensemble_grid.hip): family 2 through the materialising, mask-writing and
// selecting forms.  The materialising entry follows impnn_head_grid's order, the others go through the family's checks.
int32_t impnn_ensemble_grid_max_members(void) { return ensemble_grid_max_members(); }
int32_t impnn_ensemble_grid_max_temperatures(int32_t kind, int32_t M) { return ensemble_grid_max_temperatures(kind, M); }
int32_t impnn_ensemble_grid_topk_max_temperatures(int32_t M) { return ensemble_grid_topk_max_temperatures(M); }
int64_t impnn_ensemble_grid_tail_floats(int32_t kind, int32_t F, int32_t Mx) {
  return (kind == 0 || kind == 1) && F > 0 && Mx > 0 ? ensemble_grid_tail_floats(kind, F, Mx) : -1;
}

int impnn_ensemble_grid(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an, const float* temperatures,
                        const float* tails, float kappa, float* mean, float* std, float* score, int32_t C, int32_t A,
                        int32_t nT, int32_t F, int32_t Mx, impnn_stream_t stream) {
  const GridOperands g = ensemble_grid_operands(kind, M, mix_cat, mix_an, temperatures, tails, kappa, C, A, nT, F, Mx, stream);
  if (int rc = grid_kind_rule(__func__, g, C >= 0 && A >= 0 && nT >= 0 && F > 0 && Mx > 0)) return rc;
  if (int rc = grid_ensemble_rule(__func__, M, kappa)) return rc;
  if (int rc = head_widths_covered(__func__, 0, F, Mx)) return rc;
  if (nT > ensemble_grid_max_temperatures(kind, M))
    return fail(IMPNN_E_UNSUPPORTED, "%s: nT=%d temperatures (<= %d per call)", __func__, nT,
                ensemble_grid_max_temperatures(kind, M));
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(mix_cat && mix_an && tails && (mean || std || score) && (kind == 1 || temperatures), "null pointer");
  if (int rc = grid_no_temperatures_rule(__func__, g)) return rc;
  return launch_ensemble_grid(g, mean, std, score);
}

int impnn_ensemble_grid_mask(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                             const float* temperatures, const float* tails, float kappa, float lo, float hi,
                             uint32_t* words, int32_t C, int32_t A, int32_t nT, int32_t F, int32_t Mx,
                             impnn_stream_t stream) {
  const GridMaskCall c{ensemble_grid_operands(kind, M, mix_cat, mix_an, temperatures, tails, kappa, C, A, nT, F, Mx, stream),
                       lo, hi, words};
  return grid_mask_checked(__func__, c, F > 0 && Mx > 0, mix_cat && mix_an && tails && words && (kind == 1 || temperatures), 0);
}

int impnn_ensemble_grid_topk_workspace_bytes(int32_t M, int32_t C, int32_t A, int32_t nT, int32_t k, int32_t workgroups,
                                             size_t* need) {
  if (int rc = ensemble_topk_shape(__func__, M, 0.f, C, A, nT, k, workgroups)) return rc;
  REQUIRE(need, "null pointer");
  *need = grid_topk_workspace_bytes(2, C, A, nT, k, workgroups);
  return IMPNN_OK;
}

int impnn_ensemble_grid_topk(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                             const float* temperatures, const float* tails, float kappa, int32_t k, int32_t largest,
                             float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                             int32_t C, int32_t A, int32_t nT, int32_t F, int32_t Mx, int32_t workgroups,
                             impnn_stream_t stream) {
  const GridTopkCall c{ensemble_grid_operands(kind, M, mix_cat, mix_an, temperatures, tails, kappa, C, A, nT, F, Mx, stream),
                       k, largest, values, cation, anion, workspace, workgroups, false, nullptr};
  return grid_topk_checked(__func__, c, F > 0 && Mx > 0,
                           mix_cat && mix_an && tails && values && cation && anion && workspace && (kind == 1 || temperatures),
                           0, workspace_bytes);
}

int impnn_ensemble_grid_topk_where(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                                   const float* temperatures, const float* tails, float kappa, const uint32_t* where,
                                   int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                   void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t F,
                                   int32_t Mx, int32_t workgroups, impnn_stream_t stream) {
  const GridTopkCall c{ensemble_grid_operands(kind, M, mix_cat, mix_an, temperatures, tails, kappa, C, A, nT, F, Mx, stream),
                       k, largest, values, cation, anion, workspace, workgroups, true, where};
  return grid_topk_checked(__func__, c, F > 0 && Mx > 0,
                           mix_cat && mix_an && tails && values && cation && anion && workspace && (kind == 1 || temperatures),
                           0, workspace_bytes);
}

// ---- Monte-Carlo dropout of the transfer head over the grid (include/impnn.h; transfer_mc_grid.hip): family 3 through
// the materialising, mask-writing and selecting forms.  The materialising entry follows impnn_transfer_head_grid's
// order with S and kappa behind the shape, the others go through the family's checks.
int32_t impnn_transfer_mc_grid_max_samples(void) { return transfer_mc_grid_max_samples(); }

int impnn_transfer_mc_grid(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                           const float* multipliers, int32_t S, float kappa, float* mean, float* std, float* score,
                           float* samples, int32_t C, int32_t A, impnn_stream_t stream) {
  const GridOperands g = transfer_mc_grid_operands(u_cat, u_an, image, multipliers, S, kappa, C, A, stream);
  if (int rc = grid_kind_rule(__func__, g, C >= 0 && A >= 0 && image_floats >= 0)) return rc;
  if (int rc = grid_mc_rule(__func__, S, kappa)) return rc;
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(u_cat && u_an && image && multipliers && (mean || std || score || samples), "null pointer");
  if (int rc = grid_transfer_rule(__func__, g, image_floats)) return rc;
  return launch_transfer_mc_grid(g, mean, std, score, samples);
}

int impnn_transfer_mc_grid_mask(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                const float* multipliers, int32_t S, float kappa, float lo, float hi, uint32_t* words,
                                int32_t C, int32_t A, impnn_stream_t stream) {
  const GridMaskCall c{transfer_mc_grid_operands(u_cat, u_an, image, multipliers, S, kappa, C, A, stream), lo, hi, words};
  return grid_mask_checked(__func__, c, image_floats >= 0, u_cat && u_an && image && multipliers && words, image_floats);
}

int impnn_transfer_mc_grid_topk_workspace_bytes(int32_t S, int32_t C, int32_t A, int32_t k, int32_t workgroups,
                                                size_t* need) {
  if (int rc = mc_topk_shape(__func__, S, 0.f, C, A, k, workgroups)) return rc;
  REQUIRE(need, "null pointer");
  *need = grid_topk_workspace_bytes(3, C, A, 0, k, workgroups);
  return IMPNN_OK;
}

int impnn_transfer_mc_grid_topk(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                const float* multipliers, int32_t S, float kappa, int32_t k, int32_t largest,
                                float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                                int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream) {
  const GridTopkCall c{transfer_mc_grid_operands(u_cat, u_an, image, multipliers, S, kappa, C, A, stream), k, largest,
                       values, cation, anion, workspace, workgroups, false, nullptr};
  return grid_topk_checked(__func__, c, image_floats >= 0,
                           u_cat && u_an && image && multipliers && values && cation && anion && workspace, image_floats,
                           workspace_bytes);
}

int impnn_transfer_mc_grid_topk_where(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                      const float* multipliers, int32_t S, float kappa, const uint32_t* where,
                                      int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                      void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups,
                                      impnn_stream_t stream) {
  const GridTopkCall c{transfer_mc_grid_operands(u_cat, u_an, image, multipliers, S, kappa, C, A, stream), k, largest,
                       values, cation, anion, workspace, workgroups, true, where};
  return grid_topk_checked(__func__, c, image_floats >= 0,
                           u_cat && u_an && image && multipliers && values && cation && anion && workspace, image_floats,
                           workspace_bytes);
}

// ---- per-ion statistics of the grid (include/impnn.h; grid_summary.hip): every family through the summary form.  The
// partners entries' order: kind and shape (with M / S and kappa, carry and the plane limit), the widths, zero work, null
// pointers (the table and its seven entries), alignment and the image size, the workspace size.
namespace {
int grid_summary_planes(const GridOperands& g) { return g.nT > 0 ? g.nT : 1; }

int grid_summary_checked(const char* entry, const GridOperands& g, bool shape_ok, bool pointers_ok, int64_t image_floats,
                         const uint32_t* where, int carry, size_t workspace_bytes, const void* const* buffers) {
  if (int rc = grid_kind_rule(entry, g, shape_ok)) return rc;
  if (g.family == 2)
    if (int rc = grid_ensemble_rule(entry, g.M, g.kappa)) return rc;
  if (g.family == 3)
    if (int rc = grid_mc_rule(entry, g.M, g.kappa)) return rc;
  if (g.C < 0 || g.A < 0 || g.nT < 0) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (carry != 0 && carry != 1) return fail(IMPNN_E_BADARG, "%s: carry must be 0 or 1", entry);
  const int most = grid_summary_max_planes(g.family, g.M);
  if (g.nT > most) return fail(IMPNN_E_UNSUPPORTED, "%s: nT=%d temperatures (<= %d per call)", entry, g.nT, most);
  bool table_ok = buffers != nullptr;
  for (int i = 0; table_ok && i < 7; ++i) table_ok = buffers[i] != nullptr;
  bool launch;
  if (int rc = grid_selecting_rules(entry, g, pointers_ok && table_ok, table_ok ? buffers[6] : nullptr, where, image_floats,
                                    grid_summary_workspace_bytes(g.family, g.C, g.A, grid_summary_planes(g)),
                                    workspace_bytes, &launch))
    return rc;
  if (!launch) return IMPNN_OK;
  if (int rc = grid_aligned_rule(entry, buffers[1], buffers[4], 8, "the sums must be 8-byte aligned")) return rc;
  for (int i : {0, 2, 3, 5})
    if (int rc = grid_aligned_rule(entry, buffers[i], nullptr, 4, "the counts and the ranges must be 4-byte aligned")) return rc;
  auto at = [&](int i) { return const_cast<void*>(buffers[i]); };
  return launch_grid_summary(GridSummaryCall{g, where, carry, static_cast<uint32_t*>(at(0)), static_cast<double*>(at(1)),
                                             static_cast<float*>(at(2)), static_cast<uint32_t*>(at(3)),
                                             static_cast<double*>(at(4)), static_cast<float*>(at(5)), at(6)});
}
}  // namespace

int64_t impnn_grid_summary_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t planes) {
  if (family < 0 || family > 3 || C < 0 || A < 0 || planes < 1) return 0;
  if (planes > grid_summary_max_planes(family, family == 2 ? ensemble_grid_max_members() : 1)) return 0;  // (the fullest ensemble)
  return (int64_t)grid_summary_workspace_bytes(family, C, A, planes);
}

int impnn_head_grid_summary(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                            const float* head_weights, const uint32_t* where, int32_t carry, size_t workspace_bytes,
                            const void* const* buffers, int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F,
                            int32_t Mx, impnn_stream_t stream) {
  return grid_summary_checked(__func__,
                              head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, C, A, nT, D, F, Mx, stream),
                              D > 0 && F > 0 && Mx > 0, mix_cat && mix_an && head_weights && (kind == 1 || temperatures), 0,
                              where, carry, workspace_bytes, buffers);
}

int impnn_transfer_head_grid_summary(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                     const uint32_t* where, int32_t carry, size_t workspace_bytes,
                                     const void* const* buffers, int32_t C, int32_t A, impnn_stream_t stream) {
  return grid_summary_checked(__func__, transfer_grid_operands(u_cat, u_an, image, C, A, stream), image_floats >= 0,
                              u_cat && u_an && image, image_floats, where, carry, workspace_bytes, buffers);
}

int impnn_deep_ensemble_grid_summary(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                                const float* temperatures, const float* tails, float kappa, const uint32_t* where,
                                int32_t carry, size_t workspace_bytes, const void* const* buffers, int32_t C, int32_t A,
                                int32_t nT, int32_t F, int32_t Mx, impnn_stream_t stream) {
  return grid_summary_checked(__func__,
                              ensemble_grid_operands(kind, M, mix_cat, mix_an, temperatures, tails, kappa, C, A, nT, F, Mx, stream),
                              F > 0 && Mx > 0, mix_cat && mix_an && tails && (kind == 1 || temperatures), 0, where, carry,
                              workspace_bytes, buffers);
}

int impnn_transfer_mc_grid_summary(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                   const float* multipliers, int32_t S, float kappa, const uint32_t* where, int32_t carry,
                                   size_t workspace_bytes, const void* const* buffers, int32_t C, int32_t A,
                                   impnn_stream_t stream) {
  return grid_summary_checked(__func__, transfer_mc_grid_operands(u_cat, u_an, image, multipliers, S, kappa, C, A, stream),
                              image_floats >= 0, u_cat && u_an && image && multipliers, image_floats, where, carry,
                              workspace_bytes, buffers);
}

// ---- the applicability domain (include/impnn.h; grid_domain.hip).  The three entries' order: shape (sizes, R >= 1,
// Mx >= 1, exclude_self with Q != R, a NaN bound), the width limit, zero work, null pointers, then the launcher's tile count.
namespace {
int domain_shape_rule(const char* entry, bool sizes_ok, int R, int Mx) {
  if (!sizes_ok || Mx < 1) return fail(IMPNN_E_BADARG, "%s: bad shape", entry);
  if (R < 1) return fail(IMPNN_E_BADARG, "%s: R=%d reference rows must be at least 1", entry, R);
  return IMPNN_OK;
}
int domain_width_rule(const char* entry, int Mx) {
  if (Mx > kHeadMaxDim) return fail(IMPNN_E_UNSUPPORTED, "%s: Mx=%d (<= %d)", entry, Mx, kHeadMaxDim);
  return IMPNN_OK;
}
}  // namespace

int32_t impnn_domain_reference_chunk(void) { return domain_reference_chunk(); }

int impnn_domain_grid(const float* mix_cat, const float* mix_an, const float* ref, float* distance, int32_t* nearest,
                      int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream) {
  if (int rc = domain_shape_rule(__func__, C >= 0 && A >= 0, R, Mx)) return rc;
  if (int rc = domain_width_rule(__func__, Mx)) return rc;
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(mix_cat && mix_an && ref && distance, "null pointer");
  return launch_domain_grid(DomainGridCall{mix_cat, mix_an, ref, distance, nearest, nullptr, 0.f, 0.f, C, A, R, Mx,
                                           as_stream(stream)});
}

int impnn_domain_grid_mask(const float* mix_cat, const float* mix_an, const float* ref, float lo, float hi,
                           uint32_t* words, int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream) {
  if (int rc = domain_shape_rule(__func__, C >= 0 && A >= 0, R, Mx)) return rc;
  REQUIRE(lo == lo && hi == hi, "a bound is NaN (an infinity means no limit)");
  if (int rc = domain_width_rule(__func__, Mx)) return rc;
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(mix_cat && mix_an && ref && words, "null pointer");
  return launch_domain_grid(DomainGridCall{mix_cat, mix_an, ref, nullptr, nullptr, words, lo, hi, C, A, R, Mx,
                                           as_stream(stream)});
}

int impnn_domain_rows(const float* z, const float* ref, int32_t exclude_self, float* distance, int32_t* nearest,
                      int32_t Q, int32_t R, int32_t Mx, impnn_stream_t stream) {
  if (int rc = domain_shape_rule(__func__, Q >= 0, R, Mx)) return rc;
  REQUIRE(!exclude_self || Q == R, "exclude_self needs the queries to be the reference rows: Q == R");
  if (int rc = domain_width_rule(__func__, Mx)) return rc;
  if (Q == 0) return IMPNN_OK;
  REQUIRE(z && ref && distance, "null pointer");
  return launch_domain_rows(DomainRowsCall{z, ref, exclude_self != 0, distance, nearest, Q, R, Mx, as_stream(stream)});
}

// ---- the diverse batch (include/impnn.h; grid_diverse.hip).  The domain entries' order, with k beside the shape and
// the limits: shape and k < 1, the width, k and pair-count limits, zero work, null pointers, alignment, the workspace size.
namespace {
int diverse_shape_rule(const char* entry, int C, int A, int R, int Mx, int k) {
  if (int rc = domain_shape_rule(entry, C >= 0 && A >= 0, R, Mx)) return rc;
  if (k < 1) return fail(IMPNN_E_BADARG, "%s: k=%d must be at least 1", entry, k);
  if (int rc = domain_width_rule(entry, Mx)) return rc;
  if (k > kDiverseMaxK) return fail(IMPNN_E_UNSUPPORTED, "%s: k=%d picks (<= %d per call)", entry, k, kDiverseMaxK);
  return grid_pairs_rule(entry, C, A);
}
}  // namespace

int32_t impnn_diverse_max_k(void) { return kDiverseMaxK; }

int impnn_diverse_workspace_bytes(int32_t C, int32_t A, int32_t k, size_t* need) {
  if (int rc = diverse_shape_rule(__func__, C, A, 1, 1, k)) return rc;
  REQUIRE(need, "null pointer");
  *need = diverse_workspace_bytes(C, A, k);
  return IMPNN_OK;
}

int impnn_diverse_select(const float* mix_cat, const float* mix_an, const float* ref, const uint32_t* where, int32_t k,
                         int32_t* cation, int32_t* anion, float* distance, int64_t* counts, void* workspace,
                         size_t workspace_bytes, int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream) {
  if (int rc = diverse_shape_rule(__func__, C, A, R, Mx, k)) return rc;
  if (C == 0 || A == 0) return IMPNN_OK;
  REQUIRE(mix_cat && mix_an && ref && cation && anion && distance && counts && workspace, "null pointer");
  if (int rc = grid_aligned_rule(__func__, workspace, nullptr, 16, "the workspace must be 16-byte aligned")) return rc;
  if (int rc = grid_aligned_rule(__func__, counts, nullptr, 8, "the counts must be 8-byte aligned")) return rc;
  if (int rc = grid_aligned_rule(__func__, where, nullptr, 4, "the mask must be 4-byte aligned")) return rc;
  if (int rc = grid_workspace_rule(__func__, workspace_bytes, diverse_workspace_bytes(C, A, k))) return rc;
  return launch_diverse_select(DiverseCall{mix_cat, mix_an, ref, where, k, cation, anion, distance, counts, workspace, C,
                                           A, R, Mx, as_stream(stream)});
}

int impnn_gather_rows(int32_t n_tensors, const void* const* src, void* const* dst, const int64_t* row_bytes,
                      const int64_t* rows, int32_t n_rows, impnn_stream_t stream) {
  REQUIRE(n_tensors >= 0 && n_rows >= 0, "bad shape");
  if (n_tensors == 0 || n_rows == 0) return IMPNN_OK;
  REQUIRE(src && dst && row_bytes && rows, "null pointer");
  return launch_gather_rows(n_tensors, src, dst, row_bytes, rows, n_rows, as_stream(stream));
}

int impnn_state_rows(int32_t n_ions, const float* const* tables, const int32_t* const* rows, float* const* out,
                     const int64_t* row_floats, const int64_t* table_rows, int32_t B, impnn_stream_t stream) {
  REQUIRE(n_ions >= 1 && n_ions <= 2, "n_ions must be 1 or 2");
  REQUIRE(B >= 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(tables && rows && out && row_floats && table_rows, "null pointer");
  for (int t = 0; t < n_ions; ++t) {
    REQUIRE(tables[t] && rows[t] && out[t], "null pointer");
    REQUIRE(row_floats[t] > 0 && row_floats[t] % 4 == 0, "row_floats must be a positive multiple of 4");
    REQUIRE(table_rows[t] >= 0, "table_rows must not be negative");
    REQUIRE(((reinterpret_cast<uintptr_t>(tables[t]) | reinterpret_cast<uintptr_t>(out[t])) & 15u) == 0,
            "tables and out must be 16-byte aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(rows[t]) & 3u) == 0, "rows must be 4-byte aligned");
  }
  return launch_state_rows(n_ions, tables, rows, out, row_floats, table_rows, B, as_stream(stream));
}

int impnn_profile_enable(int32_t capacity) {
  REQUIRE(capacity > 0 && capacity <= (1 << 20), "capacity out of range");
  impnn_profile_disable();
  g_prof.start.resize(capacity);
  g_prof.stop.resize(capacity);
  for (int i = 0; i < capacity; ++i) {
    if (hipEventCreate(&g_prof.start[i]) != hipSuccess || hipEventCreate(&g_prof.stop[i]) != hipSuccess) {
      g_prof.start.resize(i);
      g_prof.stop.resize(i);
      impnn_profile_disable();
      return fail(IMPNN_E_LAUNCH, "impnn_profile_enable: hipEventCreate failed");
    }
  }
  g_prof.used = 0;
  g_prof.open = false;
  g_prof.enabled = true;
  return IMPNN_OK;
}

int impnn_profile_collect(float* ms_out, int32_t max_n, int32_t* n_out) {
  REQUIRE(n_out && (ms_out || max_n == 0) && max_n >= 0, "bad arguments");
  int n = g_prof.used < max_n ? g_prof.used : max_n;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof.stop[i]) != hipSuccess ||
        hipEventElapsedTime(&ms_out[i], g_prof.start[i], g_prof.stop[i]) != hipSuccess)
      return fail(IMPNN_E_LAUNCH, "impnn_profile_collect: event %d not readable", i);
  }
  *n_out = n;
  g_prof.used = 0;
  g_prof.open = false;
  return IMPNN_OK;
}

int impnn_profile_disable(void) {
  for (auto e : g_prof.start) (void)hipEventDestroy(e);
  for (auto e : g_prof.stop) (void)hipEventDestroy(e);
  g_prof.start.clear();
  g_prof.stop.clear();
  g_prof.used = 0;
  g_prof.enabled = false;
  g_prof.open = false;
  return IMPNN_OK;
}

int impnn_debug_set_stamp_buffer(void* device_buffer, size_t bytes) {
  g_stamp_ptr = device_buffer;
  g_stamp_bytes = device_buffer ? bytes : 0;
  return IMPNN_OK;
}

int impnn_embed_gather_bwd(const int32_t* ids, const float* dout, float* dtable, int64_t rows, int32_t vocab,
                           int32_t dim, impnn_stream_t stream) {
  REQUIRE(rows >= 0 && vocab > 0 && dim > 0, "bad shape");
  if (rows == 0) return IMPNN_OK;
  REQUIRE(ids && dout && dtable, "null pointer");
  return launch_embed_gather_bwd(ids, dout, dtable, rows, vocab, dim, as_stream(stream));
}

int impnn_embed_rows_bwd(const int32_t* ids, const float* dout, const int32_t* row_list, int32_t n_listed,
                         const void* const* buffers, int64_t rows, int32_t vocab, int32_t dim, int32_t accumulate,
                         impnn_stream_t stream) {
  REQUIRE(rows >= 0 && vocab > 0 && dim >= 0 && n_listed >= 0 && (accumulate == 0 || accumulate == 1), "bad shape");
  REQUIRE(ids || rows == vocab, "ids == NULL is the identity: rows must equal vocab");
  if (n_listed == 0 || rows == 0 || dim == 0) return IMPNN_OK;
  REQUIRE(buffers && buffers[0] && dout && row_list, "null pointer");
  float* dtable = static_cast<float*>(const_cast<void*>(buffers[0]));
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
  REQUIRE(!(misaligned(ids) || misaligned(dout) || misaligned(row_list) || misaligned(dtable)),
          "ids, dout, row_list and dtable must be 4-byte aligned");
  return launch_embed_rows_bwd(ids, dout, row_list, n_listed, dtable, rows, vocab, dim, accumulate, as_stream(stream));
}

int impnn_reduce_scatter_bwd(const float* dagg, const int32_t* tgt, int32_t tgt_stride, float* dmessages, int32_t B,
                             int32_t N, int32_t E, int32_t D, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && E >= 0 && D > 0 && tgt_stride >= 1, "bad shape");
  if (B == 0 || E == 0) return IMPNN_OK;
  REQUIRE(dagg && tgt && dmessages, "null pointer");
  return launch_reduce_scatter_bwd(dagg, tgt, tgt_stride, dmessages, B, N, E, D, as_stream(stream));
}

int impnn_global_sum_pool_bwd(const float* dpooled, const int32_t* atom_ids, float* dh, int32_t B, int32_t N,
                              int32_t D, impnn_stream_t stream) {
  REQUIRE(B >= 0 && N > 0 && D > 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  REQUIRE(dpooled && atom_ids && dh, "null pointer");
  return launch_global_sum_pool_bwd(dpooled, atom_ids, dh, B, N, D, as_stream(stream));
}

int64_t impnn_bmm_message_typed_bwd_workspace_bytes(int32_t B, int32_t E, int32_t Vb) {
  if (B < 0 || E < 0 || Vb <= 0) return 0;
  return 4 * bmm_message_typed_bwd_workspace_ints(B, E, Vb);
}

int impnn_bmm_message_typed_sorted(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                   const float* type_mats, float* messages, void* workspace, int64_t workspace_bytes,
                                   int32_t B, int32_t N, int32_t E, int32_t D, int32_t Vb, int32_t sorted_ready,
                                   impnn_stream_t stream) {
  TypedMessageCall c = typed_message(__func__, h, bond_ids, conn, type_mats, workspace, workspace_bytes, B, N, E, D, Vb,
                                     sorted_ready & 1, stream);
  c.messages = messages, c.zero_rows_ready = (sorted_ready & 2) != 0;
  return typed_message_checked(c, messages != nullptr, launch_bmm_message_typed_sorted);
}

int impnn_bmm_message_typed_bwd(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                const float* type_mats, const float* dmessages, float* dh, float* dtype_mats,
                                void* workspace, int64_t workspace_bytes, int32_t B, int32_t N, int32_t E, int32_t D,
                                int32_t Vb, int32_t sorted_ready, impnn_stream_t stream) {
  TypedMessageCall c = typed_message(__func__, h, bond_ids, conn, type_mats, workspace, workspace_bytes, B, N, E, D, Vb,
                                     sorted_ready, stream);
  c.grad = dmessages, c.dh = dh, c.dtype_mats = dtype_mats;
  return typed_message_checked(c, dmessages && dh && dtype_mats, launch_bmm_message_typed_bwd);
}

int impnn_message_reduce_typed_bwd(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                   const float* type_mats, const float* dagg, float* dh, float* dtype_mats,
                                   void* workspace, int64_t workspace_bytes, int32_t B, int32_t N, int32_t E, int32_t D,
                                   int32_t Vb, int32_t sorted_ready, impnn_stream_t stream) {
  TypedMessageCall c = typed_message(__func__, h, bond_ids, conn, type_mats, workspace, workspace_bytes, B, N, E, D, Vb,
                                     sorted_ready, stream);
  c.grad = dagg, c.dh = dh, c.dtype_mats = dtype_mats, c.from_agg = true;
  return typed_message_checked(c, dagg && dh && dtype_mats, launch_bmm_message_typed_bwd);
}

int impnn_message_reduce_typed_bwd_scratch(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                           const float* type_mats, const float* dagg, float* dh, float* dtype_mats,
                                           void* workspace, int64_t workspace_bytes, float* edge_scratch, int32_t B,
                                           int32_t N, int32_t E, int32_t D, int32_t Vb, int32_t sorted_ready,
                                           impnn_stream_t stream) {
  TypedMessageCall c = typed_message(__func__, h, bond_ids, conn, type_mats, workspace, workspace_bytes, B, N, E, D, Vb,
                                     sorted_ready, stream);
  c.grad = dagg, c.dh = dh, c.dtype_mats = dtype_mats, c.from_agg = true, c.edge_scratch = edge_scratch;
  return typed_message_checked(c, dagg && dh && dtype_mats && edge_scratch, launch_bmm_message_typed_bwd);
}

int impnn_bond_type_matrices_bwd(const float* bond_table, const float* W, const float* dtype_mats, float* dW,
                                 float* dbond_table, int32_t Vb, int32_t K, int32_t D, int32_t accumulate,
                                 impnn_stream_t stream) {
  REQUIRE(Vb > 0 && K > 0 && D > 0, "bad shape");
  REQUIRE(bond_table && W && dtype_mats && dW && dbond_table, "null pointer");
  return launch_bond_type_matrices_bwd(bond_table, W, dtype_mats, dW, dbond_table, Vb, K, D, accumulate != 0,
                                       as_stream(stream));
}

int impnn_bond_type_matrices_multi(const float* bond_table, const float* const* W, float* const* type_mats, int32_t n,
                                   int32_t Vb, int32_t K, int32_t D, impnn_stream_t stream) {
  REQUIRE(n >= 0 && Vb > 0 && K > 0 && D > 0, "bad shape");
  if (n == 0) return IMPNN_OK;
  REQUIRE(bond_table && W && type_mats, "null pointer");
  return launch_bond_type_matrices_multi(bond_table, W, type_mats, n, Vb, K, D, as_stream(stream));
}

int impnn_bond_type_matrices_multi_bwd(const float* bond_table, const float* const* W, const float* const* dtype_mats,
                                       float* const* dW, float* dbond_table, int32_t n, int32_t Vb, int32_t K,
                                       int32_t D, int32_t accumulate, impnn_stream_t stream) {
  REQUIRE(n >= 0 && Vb > 0 && K > 0 && D > 0, "bad shape");
  if (n == 0) return IMPNN_OK;
  REQUIRE(bond_table && W && dtype_mats && dW && dbond_table, "null pointer");
  return launch_bond_type_matrices_multi_bwd(bond_table, W, dtype_mats, dW, dbond_table, n, Vb, K, D, accumulate != 0,
                                             as_stream(stream));
}

int64_t impnn_bond_type_matrices_multi_bwd_workspace_floats(int32_t n, int32_t Vb, int32_t K, int32_t D) {
  if (n <= 0 || Vb <= 0 || K <= 0 || D <= 0) return 0;
  return bond_type_matrices_multi_bwd_workspace(n, Vb, K, D);
}

int impnn_bond_type_matrices_multi_bwd_ws(const float* bond_table, const float* const* W,
                                          const float* const* dtype_mats, float* const* dW, float* dbond_table,
                                          int32_t n, int32_t Vb, int32_t K, int32_t D, int32_t accumulate,
                                          float* workspace, int64_t workspace_floats, impnn_stream_t stream) {
  REQUIRE(n >= 0 && Vb > 0 && K > 0 && D > 0, "bad shape");
  if (n == 0) return IMPNN_OK;
  REQUIRE(bond_table && W && dtype_mats && dW && dbond_table && workspace, "null pointer");
  if (workspace_floats < impnn_bond_type_matrices_multi_bwd_workspace_floats(n, Vb, K, D))
    return fail(IMPNN_E_WORKSPACE, "bond_type_matrices_multi_bwd_ws: workspace of %lld floats is too small",
                (long long)workspace_floats);
  return launch_bond_type_matrices_multi_bwd(bond_table, W, dtype_mats, dW, dbond_table, n, Vb, K, D, accumulate != 0,
                                             as_stream(stream), workspace);
}

int64_t impnn_gated_update_param_floats(int32_t D) { return D > 0 ? gated_update_param_floats(D) : 0; }

int64_t impnn_gated_update_bwd_workspace_floats(int64_t rows, int32_t D) {
  if (rows < 0 || D <= 0) return 0;
  return gated_update_bwd_workspace(rows, D);
}

int64_t impnn_gated_update_rows_bwd_workspace_floats(int64_t max_rows, int32_t D) {
  if (max_rows < 0 || (D != 64 && D != 128)) return 0;
  return gated_update_bwd_workspace(max_rows, D, true);
}

int64_t impnn_gated_update_rows_saved_floats(int64_t max_rows, int32_t D) {
  if (max_rows < 0 || (D != 32 && D != 64 && D != 128)) return 0;
  return max_rows * 4 * D;
}

int impnn_gated_update(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                       const float* br, const float* Wh, const float* bh, const float* gamma,
                       const float* beta, float ln_eps, float* out, int64_t rows, int32_t D,
                       impnn_stream_t stream) {
  return gated_update_checked(gu_forward(__func__, kFwd, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, ln_eps, out, nullptr, nullptr, rows, D, nullptr, stream));
}

int impnn_gated_update_rows(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                            const float* br, const float* Wh, const float* bh, const float* gamma,
                            const float* beta, float ln_eps, float* out, const int32_t* row_index,
                            const int32_t* n_rows, int64_t max_rows, int32_t D, impnn_stream_t stream) {
  return gated_update_checked(
      gu_forward(__func__, kFwdRows, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, ln_eps, out, row_index, n_rows, max_rows, D, nullptr, stream));
}

int impnn_gated_update_rows_train(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                                  const float* br, const float* Wh, const float* bh, const float* gamma,
                                  const float* beta, float ln_eps, float* out, const int32_t* row_index,
                                  const int32_t* n_rows, int64_t max_rows, int32_t D, float* saved,
                                  impnn_stream_t stream) {
  return gated_update_checked(
      gu_forward(__func__, kFwdTrain, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, ln_eps, out, row_index, n_rows, max_rows, D, saved, stream));
}

int impnn_gated_update_dropout(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                               const float* br, const float* Wh, const float* bh, const float* gamma,
                               const float* beta, float ln_eps, float* out, int64_t rows, int32_t D, float rate,
                               uint64_t seed, const int64_t* step, int32_t layer_word, impnn_stream_t stream) {
  GatedUpdateCall c = gu_forward(__func__, kFwd, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, ln_eps, out, nullptr, nullptr, rows, D, nullptr, stream);
  if (int rc = add_dropout(c, rate, seed, step, layer_word)) return rc;
  return gated_update_checked(c);
}

int impnn_gated_update_rows_train_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                          const float* Wr, const float* br, const float* Wh, const float* bh,
                                          const float* gamma, const float* beta, float ln_eps, float* out,
                                          const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                          float* saved, float rate, uint64_t seed, const int64_t* step,
                                          int32_t layer_word, impnn_stream_t stream) {
  // rate 0 is the plain entry these arguments name: the saving forward, the row list, or every row
  const GatedUpdateForm form = rate != 0.f ? kFwdTrainDropout : saved ? kFwdTrain : row_index ? kFwdRows : kFwd;
  GatedUpdateCall c = gu_forward(__func__, form, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, ln_eps, out, row_index, n_rows, max_rows, D, saved, stream);
  if (int rc = add_dropout(c, rate, seed, step, layer_word)) return rc;
  return gated_update_checked(c);
}

int impnn_gated_update_bwd(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                           const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                           const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                           int64_t workspace_floats, int64_t rows, int32_t D, int32_t accumulate,
                           impnn_stream_t stream) {
  return gated_update_bwd_checked(
      gu_backward(__func__, kBwd, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, nullptr, nullptr, rows, D, accumulate, nullptr, stream));
}

int impnn_gated_update_rows_bwd(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                                const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                                const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                                int64_t workspace_floats, const int32_t* row_index, const int32_t* n_rows,
                                int64_t max_rows, int32_t D, int32_t accumulate, impnn_stream_t stream) {
  return gated_update_bwd_checked(
      gu_backward(__func__, kBwdRows, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, row_index, n_rows, max_rows, D, accumulate, nullptr, stream));
}

int impnn_gated_update_rows_bwd_saved(const float* h, const float* agg, const float* Wz, const float* bz,
                                      const float* Wr, const float* br, const float* Wh, const float* bh,
                                      const float* gamma, float ln_eps, const float* dout, float* dh, float* dagg,
                                      float* dparams, float* workspace, int64_t workspace_floats,
                                      const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                      int32_t accumulate, float* saved, impnn_stream_t stream) {
  return gated_update_bwd_checked(
      gu_backward(__func__, kBwdSaved, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, row_index, n_rows, max_rows, D, accumulate, saved, stream));
}

int impnn_gated_update_bwd_dropout(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                                   const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                                   const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                                   int64_t workspace_floats, int64_t rows, int32_t D, int32_t accumulate, float rate,
                                   uint64_t seed, const int64_t* step, int32_t layer_word, impnn_stream_t stream) {
  GatedUpdateCall c = gu_backward(__func__, kBwd, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, nullptr, nullptr, rows, D, accumulate, nullptr, stream);
  if (int rc = add_dropout(c, rate, seed, step, layer_word)) return rc;
  return gated_update_bwd_checked(c);
}

int impnn_gated_update_rows_bwd_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                        const float* Wr, const float* br, const float* Wh, const float* bh,
                                        const float* gamma, float ln_eps, const float* dout, float* dh, float* dagg,
                                        float* dparams, float* workspace, int64_t workspace_floats,
                                        const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                        int32_t accumulate, float rate, uint64_t seed, const int64_t* step,
                                        int32_t layer_word, impnn_stream_t stream) {
  GatedUpdateCall c =
      gu_backward(__func__, kBwdRows, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, row_index, n_rows, max_rows, D, accumulate, nullptr, stream);
  if (int rc = add_dropout(c, rate, seed, step, layer_word)) return rc;
  return gated_update_bwd_checked(c);
}

int impnn_gated_update_rows_bwd_saved_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                              const float* Wr, const float* br, const float* Wh, const float* bh,
                                              const float* gamma, float ln_eps, const float* dout, float* dh,
                                              float* dagg, float* dparams, float* workspace, int64_t workspace_floats,
                                              const int32_t* row_index, const int32_t* n_rows, int64_t max_rows,
                                              int32_t D, int32_t accumulate, float* saved, float rate, uint64_t seed,
                                              const int64_t* step, int32_t layer_word, impnn_stream_t stream) {
  GatedUpdateCall c =
      gu_backward(__func__, kBwdSaved, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, ln_eps, dout, dh, dagg, dparams, workspace, workspace_floats, row_index, n_rows, max_rows, D, accumulate, saved, stream);
  if (int rc = add_dropout(c, rate, seed, step, layer_word)) return rc;
  return gated_update_bwd_checked(c);
}

int impnn_dropout_step(int64_t* counter, int64_t* snapshot, impnn_stream_t stream) {
  REQUIRE(counter && snapshot, "null pointer");
  return launch_dropout_step(counter, snapshot, as_stream(stream));
}

int impnn_dropout_mask(uint64_t seed, const int64_t* step, int32_t layer_word, float rate, const int32_t* row_index,
                       const int32_t* n_rows, int64_t max_rows, int32_t D, float* out, impnn_stream_t stream) {
  DropoutArgs d;
  if (int rc = check_dropout(__func__, rate, seed, step, layer_word, &d)) return rc;
  REQUIRE(max_rows >= 0 && D > 0, "bad shape");
  REQUIRE((row_index != nullptr) == (n_rows != nullptr), "row_index and n_rows: both or neither");
  if (max_rows == 0) return IMPNN_OK;
  REQUIRE(out, "null pointer");
  return launch_dropout_mask(d, row_index, n_rows, max_rows, D, out, as_stream(stream));
}

int impnn_adam_clipnorm_step(const void* var_table, const int64_t* sizes, int32_t n_vars, int64_t step, float lr,
                             float beta1, float beta2, float eps, float clipnorm, impnn_stream_t stream) {
  REQUIRE(n_vars >= 0 && step >= 1, "bad arguments (step counts from 1)");
  if (n_vars == 0) return IMPNN_OK;
  REQUIRE(var_table && sizes, "null pointer");
  return launch_adam_clipnorm(var_table, sizes, n_vars, step, nullptr, lr, beta1, beta2, eps, clipnorm,
                              as_stream(stream));
}

int impnn_adam_clipnorm_step_counted(const void* var_table, const int64_t* sizes, int32_t n_vars, int64_t* step_counter,
                                     float lr, float beta1, float beta2, float eps, float clipnorm,
                                     impnn_stream_t stream) {
  REQUIRE(n_vars >= 0, "bad arguments");
  REQUIRE(var_table && sizes && step_counter, "null pointer");
  return launch_adam_clipnorm(var_table, sizes, n_vars, 0, step_counter, lr, beta1, beta2, eps, clipnorm,
                              as_stream(stream));
}

int impnn_lr_schedule_check(const void* host_record) {
  REQUIRE(host_record, "null pointer");
  int32_t r[kLrWords];
  std::memcpy(r, host_record, sizeof(r));
  const auto f = [&](int i) { float x; std::memcpy(&x, &r[i], 4); return x; };
  const auto finite = [](float x) { return x - x == 0.f; };
  if (r[kLrKind] < kLrConstant || r[kLrKind] > kLrPiecewise)
    return fail(IMPNN_E_UNSUPPORTED, "%s: unknown schedule kind %d", __func__, r[kLrKind]);
  REQUIRE(finite(f(kLrBase)), "the base rate is not finite");
  if (r[kLrKind] == kLrExponential || r[kLrKind] == kLrCosine) {
    REQUIRE(r[kLrDecaySteps] > 0, "decay_steps must be > 0");
    REQUIRE(finite(f(kLrParam)), "decay_rate / alpha is not finite");
  }
  if (r[kLrKind] == kLrExponential) REQUIRE(f(kLrParam) >= 0.f, "decay_rate must be >= 0");
  if (r[kLrKind] == kLrCosine) REQUIRE(r[kLrWarmupSteps] >= 0 && finite(f(kLrTarget)), "bad warm-up");
  if (r[kLrKind] == kLrPiecewise) {
    if (r[kLrBoundaryCount] < 0 || r[kLrBoundaryCount] > kLrMaxBoundaries)
      return fail(IMPNN_E_UNSUPPORTED, "%s: %d boundaries (at most %d)", __func__, r[kLrBoundaryCount], kLrMaxBoundaries);
    for (int i = 0; i + 1 < r[kLrBoundaryCount]; ++i)
      REQUIRE(r[kLrBoundaries + i] < r[kLrBoundaries + i + 1], "boundaries must increase");
    for (int i = 0; i <= r[kLrBoundaryCount]; ++i) REQUIRE(finite(f(kLrValues + i)), "a value is not finite");
  }
  return IMPNN_OK;
}

int impnn_lr_schedule_eval(const void* record, const int64_t* steps, float* out, int32_t n, impnn_stream_t stream) {
  REQUIRE(n >= 0, "bad count");
  if (n == 0) return IMPNN_OK;
  REQUIRE(record && steps && out, "null pointer");
  REQUIRE((reinterpret_cast<uintptr_t>(record) & 3u) == 0, "the record must be 4-byte aligned");
  return launch_lr_schedule_eval(record, steps, out, n, as_stream(stream));
}

int64_t impnn_adam_step_scheduled_workspace_floats(int32_t n_vars) { return adam_scheduled_workspace(n_vars); }

int impnn_adam_step_scheduled(const void* var_table, const int64_t* sizes, int32_t n_vars, int64_t* step_counter,
                              const void* lr_record, float beta1, float beta2, float eps, float clipnorm,
                              float global_clipnorm, float weight_decay, const int32_t* decay_flags, float* workspace,
                              int64_t workspace_floats, impnn_stream_t stream) {
  REQUIRE(n_vars >= 0, "bad arguments");
  REQUIRE(!(clipnorm > 0.f && global_clipnorm > 0.f), "clipnorm and global_clipnorm exclude each other");
  REQUIRE(weight_decay >= 0.f && weight_decay - weight_decay == 0.f, "weight_decay must be finite and >= 0");
  if (n_vars == 0) return IMPNN_OK;
  REQUIRE(var_table && sizes && step_counter && lr_record, "null pointer");
  REQUIRE((reinterpret_cast<uintptr_t>(lr_record) & 3u) == 0, "the record must be 4-byte aligned");
  REQUIRE(!(weight_decay > 0.f) || decay_flags, "weight_decay without decay_flags");
  if (global_clipnorm > 0.f) {
    if (workspace_floats < adam_scheduled_workspace(n_vars))
      return fail(IMPNN_E_WORKSPACE, "%s: workspace of %lld floats is too small", __func__, (long long)workspace_floats);
    REQUIRE(workspace, "null workspace");
  }
  return launch_adam_scheduled(var_table, sizes, n_vars, step_counter, lr_record, beta1, beta2, eps, clipnorm,
                               global_clipnorm, weight_decay, weight_decay > 0.f ? decay_flags : nullptr,
                               workspace, as_stream(stream));
}

int impnn_batch_assemble(int32_t n_ions, const int32_t* sample_idx, int32_t B, int32_t M,
                         const int32_t* const* atom_flat, const int32_t* const* atom_off,
                         const int32_t* const* edge_flat, const int32_t* const* bond_flat,
                         const int32_t* const* edge_off, int32_t id_shift, int32_t N, int32_t L,
                         int32_t* const* atom_ids, int32_t* const* bond_ids, int32_t* const* conn,
                         const float* t_flat, float* t_out, impnn_stream_t stream) {
  REQUIRE(n_ions >= 1 && n_ions <= 2, "n_ions must be 1 or 2");
  REQUIRE(B >= 0 && M >= 1 && N >= 1 && L >= 0, "bad shape");
  REQUIRE(atom_flat && atom_off && edge_flat && bond_flat && edge_off && atom_ids && bond_ids && conn,
          "null pointer array");
  if (B == 0) return IMPNN_OK;
  REQUIRE(sample_idx, "null sample_idx");
  for (int g = 0; g < n_ions; ++g) {
    REQUIRE(atom_flat[g] && atom_off[g] && edge_off[g] && atom_ids[g], "null per-ion pointer");
    REQUIRE(L == 0 || (edge_flat[g] && bond_flat[g] && bond_ids[g] && conn[g]), "null per-ion edge pointer");
    REQUIRE((reinterpret_cast<uintptr_t>(edge_flat[g]) & 7u) == 0 && (reinterpret_cast<uintptr_t>(conn[g]) & 7u) == 0,
            "edge_flat / conn must be 8-byte aligned");
  }
  REQUIRE(!t_out || t_flat, "t_out without t_flat");
  return launch_batch_assemble(n_ions, sample_idx, B, M, atom_flat, atom_off, edge_flat, bond_flat, edge_off,
                               id_shift, N, L, atom_ids, bond_ids, conn, t_flat, t_out, as_stream(stream));
}

int impnn_validate_indices(const int32_t* conn, const int32_t* atom_ids, const int32_t* bond_ids,
                           int32_t* counts, int32_t B, int32_t N, int32_t E, int32_t Va, int32_t Vb,
                           impnn_stream_t stream) {
  REQUIRE(counts, "null pointer");
  REQUIRE(B >= 0 && N > 0 && E >= 0, "bad shape");
  if (B == 0) return IMPNN_OK;
  return launch_validate_indices(conn, atom_ids, bond_ids, counts, B, N, E, Va, Vb, as_stream(stream));
}

}  // extern "C"
