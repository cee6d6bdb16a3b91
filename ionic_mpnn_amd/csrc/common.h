// Shared host-side helpers for libimpnn.so (gfx950 only; no other target is supported).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/impnn.h"

namespace impnn {

// thread-local last-error text (impnn_last_error_string)
char* error_buffer();
int fail(int code, const char* fmt, ...);

inline hipStream_t as_stream(impnn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IMPNN_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return IMPNN_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int kWave = 64;  // CDNA wavefront

// ---- GatedUpdate dropout.  Philox4x32-10 (Salmon et al., SC'11), the counter-based generator of
// Random123: one call gives four 32-bit words.  Element (row, column) of a (rows, D) GatedUpdate output draws word
// column % 4 of philox(counter = (column / 4, row, layer_word, lo32(step)), key = (lo32(seed), hi32(seed) ^
// hi32(step))); it is kept iff (word >> 8) * 2^-24 >= rate, i.e. iff (word >> 8) >= thr = ceil(rate * 2^24), and a
// kept element is out * scale with scale = 1 / (1 - rate), a dropped one +0.  The backward regenerates the mask.
struct Philox4 {
  uint32_t v[4];
};

__device__ __host__ inline uint32_t philox_mulhi(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * b) >> 32);
}

__device__ __host__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    if (i > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// What a dropout kernel instantiation receives (by value).  `step` points at a device int64 step (a snapshot slot of
// impnn_dropout_step); the kernels read it once and never take the step from the host.
struct DropoutArgs {
  float scale;          // 1 / (1 - rate), rounded to float
  uint32_t thr;         // ceil(rate * 2^24): keep iff (word >> 8) >= thr
  uint32_t k0, k1;      // lo32(seed), hi32(seed)
  uint32_t layer_word;  // layer_id | (rank << 16)
  const int64_t* step;
};

// rate in [0, 1) -> false otherwise (NaN included)
inline bool dropout_args(float rate, uint64_t seed, const int64_t* step, int32_t layer_word, DropoutArgs* d) {
  if (!(rate >= 0.f && rate < 1.f)) return false;
  d->scale = 1.0f / (1.0f - rate);
  d->thr = (uint32_t)ceilf(rate * 16777216.0f);  // exact: a power-of-two scaling of a float below 1
  d->k0 = (uint32_t)seed;
  d->k1 = (uint32_t)(seed >> 32);
  d->layer_word = (uint32_t)layer_word;
  d->step = step;
  return true;
}

// The per-launch part of the key and counter: x2 = layer word, x3 = lo32(step), k1 ^= hi32(step).
struct DropoutKey {
  uint32_t k0, k1, x2, x3, thr;
  float scale;
};

__device__ __forceinline__ DropoutKey dropout_key(const DropoutArgs& d) {
  const int64_t st = *d.step;
  return DropoutKey{d.k0, d.k1 ^ (uint32_t)((uint64_t)st >> 32), d.layer_word, (uint32_t)st, d.thr, d.scale};
}

__device__ __forceinline__ Philox4 dropout_bits(const DropoutKey& k, int64_t row, int col4) {
  return philox4x32_10((uint32_t)col4, (uint32_t)row, k.x2, k.x3, k.k0, k.k1);
}

__device__ __forceinline__ float dropout_apply(const DropoutKey& k, uint32_t word, float v) {
  return (word >> 8) >= k.thr ? v * k.scale : 0.0f;
}

// Kernels take the dropout arguments as an optional trailing parameter pack (`class... Drop`): the instantiation
// without them has exactly the parameters, and so the code, of the kernel before dropout existed.
__device__ __forceinline__ DropoutArgs dropout_of() { return DropoutArgs{}; }
__device__ __forceinline__ DropoutArgs dropout_of(const DropoutArgs& d) { return d; }

__device__ __forceinline__ uint32_t philox_word(const Philox4& p, int i) {
  return i == 0 ? p.v[0] : i == 1 ? p.v[1] : i == 2 ? p.v[2] : p.v[3];
}

// The MFMA tile layout of the wide GatedUpdate kernels: lane j = lane & 3 of a quad of lanes owns column 4 * col4 + j
// of the quad's four rows g = 0..3 (row_j: the row with g == j).  One Philox call per lane, for row_j; a 4 x 4
// transpose across the quad then hands lane j word j of every row: w[g].  All four lanes of the quad must be active.
__device__ __forceinline__ void dropout_quad_words(const DropoutKey& k, int64_t row_j, int col4, int j, uint32_t w[4]) {
  const Philox4 p = dropout_bits(k, row_j, col4);
  uint32_t got[4];  // got[s]: word j of the row of lane j ^ s
  got[0] = philox_word(p, j);
#pragma unroll
  for (int s = 1; s < 4; ++s) got[s] = (uint32_t)__shfl_xor((int)philox_word(p, j ^ s), s);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int s = g ^ j;
    w[g] = s == 0 ? got[0] : s == 1 ? got[1] : s == 2 ? got[2] : got[3];
  }
}

// ---- one GatedUpdate call (include/impnn.h, the GatedUpdate family).  api.hip fills it from the entry's arguments
// and checks it once per direction; the launchers read it.  The form is what the entry takes and covers: whether it
// has a row list and a `saved` buffer (a form without one leaves those pointers null), and its atom_dims.
enum class GuArg : uint8_t { kAbsent, kOptional, kRequired };
enum class GuDims : uint8_t { kAny, kDivide256, k32_64_128, k64_128 };
struct GatedUpdateForm {
  GuArg row_list, saved;
  GuDims dims;
};

struct GatedUpdateCall {
  const char* entry;  // the exported entry, named by the error text
  GatedUpdateForm form;
  const float *h, *agg, *Wz, *bz, *Wr, *br, *Wh, *bh, *gamma;
  const float* beta;  // forward
  float eps;
  float* out;          // forward
  const float* dout;   // backward: dout .. accumulate
  float *dh, *dagg, *dparams, *workspace;
  int64_t workspace_floats;
  bool accumulate;
  const int32_t *row_index, *n_rows;  // the row list (device), or both null
  int64_t rows;                       // max_rows with a row list
  int D;
  float* saved;
  bool dropout;  // rate > 0: `drop` holds the mask's arguments
  DropoutArgs drop;
  hipStream_t stream;
};

// f() or f(drop): the kernels' optional trailing dropout pack (Drop... = nothing, or one DropoutArgs)
template <class F>
int with_dropout_pack(const GatedUpdateCall& c, F&& f) {
  return c.dropout ? f(c.drop) : f();
}

// ---- one typed-message call (include/impnn.h: impnn_bmm_message_typed_sorted, impnn_bmm_message_typed_bwd,
// impnn_message_reduce_typed_bwd[_scratch]).  api.hip fills it from the entry's arguments and checks it; the
// launchers (message_typed.hip) read it.
constexpr int kMaxTypes = 4096;  // bond types the family's kernels cover (their LDS histograms); also D <= 128
struct TypedMessageCall {
  const char* entry;  // the exported entry, named by the error text
  const float* h;
  const int32_t *bond_ids, *conn;
  const float* type_mats;
  float* messages;            // forward
  const float* grad;          // backward: of the messages (B,E,D), or with from_agg of Reduce's output (B,N,D)
  float *dh, *dtype_mats;     // backward: added into
  float* edge_scratch;        // backward, optional (B,E,D): per-edge vectors summed into dh in slot order, no atomics on dh
  void* workspace;            // the edge sort (EdgeSortView)
  int64_t workspace_bytes;
  int B, N, E, D, Vb;
  bool sort_ready;       // the workspace holds this batch's sort (an earlier call of the pass made it)
  bool zero_rows_ready;  // forward: `messages` still holds the zero rows of an earlier call on this batch
  bool from_agg;         // backward: `grad` is read at every edge's target row
  hipStream_t stream;
};

// The sort workspace (int32): cnt Vb+1 | start Vb+1 | cursor Vb+1 | segbase Vb+1 | order B*E
// (bmm_message_typed_bwd_workspace_ints).
struct EdgeSortView {
  int32_t *cnt, *start, *cursor, *segbase, *order;
  EdgeSortView(void* workspace, int Vb)
      : cnt(static_cast<int32_t*>(workspace)), start(cnt + Vb + 1), cursor(start + Vb + 1), segbase(cursor + Vb + 1),
        order(segbase + Vb + 1) {}
};

// ---- the widths every head kernel covers (model_head.hip, head_grid.hip, transfer_head.hip, transfer_grid.hip): LDS row
// strides as well as the limits api.hip and the launchers refuse above; ops.py mirrors them (HEAD_MAX_X, HEAD_MAX_DIM)
constexpr int kHeadMaxX = 128;   // pooled width (atom_dim)
constexpr int kHeadMaxDim = 64;  // fp_size, mixing_size
// the refusal of a width above them, in the name of an entry (api.hip: the grid families) or of a launcher (model_head.hip)
inline int head_widths_covered(const char* what, int D, int F, int Mx) {
  if (D > kHeadMaxX || F > kHeadMaxDim || Mx > kHeadMaxDim)
    return fail(IMPNN_E_UNSUPPORTED, "%s: dims D=%d (<= %d) F=%d Mx=%d (<= %d)", what, D, kHeadMaxX, F, Mx, kHeadMaxDim);
  return IMPNN_OK;
}

// ---- one model head call (include/impnn.h: impnn_model_head, _tensors, _bwd, _loss, _loss_bwd and
// impnn_weighted_model_head_loss[_bwd]).  api.hip fills it from the entry's arguments and checks it
// (model_head_checked); the launchers (model_head.hip) read it.  Pointers an entry does not take stay null; `y` is what
// makes a call a loss call.
struct ModelHeadCall {
  const char* entry;  // the exported entry, named by the error text
  int kind;           // 0 viscosity, 1 melting point
  const float *pc, *pa, *T;
  const float* w;               // impnn_model_head: the packed head; every other entry:
  const float* const* weights;  // 10 / 12 device pointers in the packed order (a host table)
  float* const* dweights;       // backward: the gradients, added into
  const float* dout;            // backward, plain
  float *out, *dpc, *dpa;       // forward (optional in the loss forward); backward
  const float *l2, *y, *dloss;  // loss entries: host lambdas per tensor, targets; backward: device scalar
  const float* sample_weight;   // weighted loss entries: (B) device floats next to y; null: the unweighted loss
  float *loss, *workspace;      // loss forward: device scalar; model_head_loss_workspace_floats
  int64_t workspace_floats;
  int B, D, F, Mx;
  hipStream_t stream;
};
int64_t model_head_loss_workspace_floats(int B);
int64_t model_head_bwd_max_floats();                    // the backward's LDS fit, in packed weight floats
int launch_model_head(const ModelHeadCall& c);          // a checked call (api.hip)
int launch_model_head_tensors(const ModelHeadCall& c);  // a checked call (api.hip)
int launch_model_head_bwd(const ModelHeadCall& c);      // a checked call (api.hip)

// ---- layer-at-a-time launches (layer_kernels.hip)
int launch_embed_gather(const int32_t* ids, const float* table, float* out, int64_t rows, int vocab,
                        int dim, hipStream_t s);
int launch_bmm_message(const float* h, const float* bs, const int32_t* conn, const float* W, float* m,
                       float* agg, int B, int N, int E, int D, int K, hipStream_t s);
int launch_bond_type_matrices(const float* tb, const float* W, float* out, int Vb, int K, int D,
                              hipStream_t s);
int launch_bmm_message_typed(const float* h, const int32_t* bond_ids, const int32_t* conn,
                             const float* type_mats, float* m, int B, int N, int E, int D, int Vb,
                             hipStream_t s);
int launch_reduce_scatter_add(const float* m, const int32_t* tgt, int tgt_stride, float* agg, int B,
                              int N, int E, int D, hipStream_t s, int accumulate = 0);
int launch_gated_update(const GatedUpdateCall& c);  // a checked call (api.hip)
int launch_kept_rows(const int32_t* atom_ids, const int32_t* bond_ids, const int32_t* conn, int32_t* rows_out, int B,
                     int N, int E, int Vb, hipStream_t s);
int launch_row_index_fill(const int32_t* r, const int32_t* incl, int32_t* idx, int32_t* count, int B, int N,
                          hipStream_t s);
int launch_global_sum_pool(const float* h, const int32_t* ids, float* out, int B, int N, int D,
                           hipStream_t s);
// ---- the transfer head (transfer_head.hip; include/impnn.h, impnn_transfer_head*).  api.hip fills and checks it.
constexpr int kThTensors = 18;
struct TransferHeadCall {
  const float *pc, *pa;             // (B,D) each; with cat_row: the tables (C,D), (A,D)
  const int32_t *cat_row, *an_row;  // indexed entries: (B) rows of the tables per sample; null: pc / pa hold the samples
  int C, A;                         // rows of the tables (indexed entries)
  const float* const* weights;  // kThTensors device pointers
  float* const* dweights;       // backward: kThTensors device pointers, null where a tensor is frozen
  const float* l2;              // host, kThTensors lambdas
  float *moving_mean, *moving_var;
  float bn_momentum, bn_eps;
  bool bn_batch;  // normalise with the batch statistics and move the moving ones (else: the moving statistics)
  const float* y;
  const float* sample_weight;  // (B) device floats next to y: the loss is (1/B) sum_b w_b L_b; null: unweighted
  int loss_kind;  // 0 squared error, 1 Huber(delta)
  float delta;
  const float* dloss;
  bool dropout;
  DropoutArgs drop;
  float* saved;
  float *out, *loss, *workspace;
  float *dpc, *dpa;
  int B, D, F, Mx;
  hipStream_t stream;
};
int64_t transfer_head_saved_floats(int B, int F, int Mx);
int64_t transfer_head_bwd_workspace_floats(int B, int F, int Mx);
int64_t transfer_head_loss_workspace_floats(int B);
int launch_transfer_head(const TransferHeadCall& c);
int launch_transfer_head_bwd(const TransferHeadCall& c);
int launch_gather_rows(int n, const void* const* src, void* const* dst, const int64_t* row_bytes, const int64_t* rows,
                       int n_rows, hipStream_t s);
int launch_state_rows(int n_ions, const float* const* tables, const int32_t* const* rows, float* const* out,
                      const int64_t* row_floats, const int64_t* table_rows, int B, hipStream_t s);
int launch_validate_indices(const int32_t* conn, const int32_t* atom_ids, const int32_t* bond_ids,
                            int32_t* counts, int B, int N, int E, int Va, int Vb, hipStream_t s);

// ---- the head over a cation x anion grid (head_grid.hip; include/impnn.h, impnn_head_ion_mix / impnn_head_grid).
// api.hip checks the arguments; `w` is the packed head of impnn_model_head.
int launch_head_ion_mix(int kind, int ion, const float* pooled, const float* w, float* mix, int M, int D, int F, int Mx,
                        hipStream_t s);
int head_grid_max_temperatures();

// The operands every grid launch shares (api.hip builds and checks them).  family 0: the head grid (`kind`, mixing
// rows, T, the packed head of impnn_model_head in `w`); family 1: the transfer grid (u rows in mix_cat / mix_an, the
// prepared image in `w`; kind 1, no T, no widths); family 2: the ensemble grid (`M` members of `kind`: mixing rows
// (M,C,Mx) and (M,A,Mx), T, the members' tails (M, tail floats) in `w`, `kappa` of the score; no D); family 3: the
// transfer MC grid (family 1's operands, `M` samples, their `multipliers` (M,128) and `kappa`).
struct GridOperands {
  int family, kind;
  const float *mix_cat, *mix_an, *T, *w;
  int C, A, nT, D, F, Mx;
  hipStream_t stream;
  int M;        // family 2: members; family 3: samples
  float kappa;  // families 2 and 3
  const float* multipliers;  // family 3
};
int launch_head_grid(const GridOperands& g, float* out, float* params);

// ---- the transfer head over a cation x anion grid (transfer_grid.hip; include/impnn.h, impnn_transfer_grid_prepare /
// impnn_transfer_ion_half / impnn_transfer_head_grid).  api.hip checks the arguments; `weights`: kThTensors pointers.
int64_t transfer_grid_image_floats();
int launch_transfer_grid_prepare(const float* const* weights, const float* moving_mean, const float* moving_var,
                                 float bn_eps, float* image, hipStream_t s);
int launch_transfer_ion_half(int ion, const float* pooled, const float* const* weights, float* u, int M, int D, int F,
                             int Mx, hipStream_t s);
int launch_transfer_head_grid(const GridOperands& g, float* out);

// ---- top-k selection over a cation x anion grid (grid_select.hip; include/impnn.h, impnn_head_grid_topk /
// impnn_transfer_head_grid_topk).  The limits of one selecting launch (ops.py mirrors them):
constexpr int kSelectMaxK = 1024;  // entries kept per temperature: one head_grid tile's worth
constexpr int kSelectMaxT = 4;     // temperatures: 16 KiB of LDS each beside the tile's regions
// One selecting launch.  api.hip checks the arguments.
struct GridTopkCall {
  GridOperands g;
  int k, largest;
  float* values;
  int32_t *cation, *anion;
  void* workspace;
  int workgroups;
  bool masked;            // the _where entries: only pairs whose bit of `where` is set compete
  const uint32_t* where;  // (C, ceil(A / 32)) words
};
int grid_topk_workgroups(int family, int C, int A, int workgroups);  // 0: the default; capped by the tile count
size_t grid_topk_workspace_bytes(int family, int C, int A, int nT, int k, int workgroups);
int launch_grid_topk(const GridTopkCall& c);
// the second launch of a selecting call: the G workgroups' lists in `ws` -> values, cation, anion (nT, k)
int launch_grid_topk_merge(const unsigned long long* ws, int G, int nT, int k, int largest, int A, float* values,
                           int32_t* cation, int32_t* anion, hipStream_t s);

// ---- pair masks (grid_mask.hip; include/impnn.h, impnn_head_grid_mask / impnn_transfer_head_grid_mask).  One
// mask-writing launch: bit (i, j) = lo <= prediction <= hi.  api.hip checks it.
struct GridMaskCall {
  GridOperands g;
  float lo, hi;
  uint32_t* words;  // (C, W), viscosity (nT, C, W); W = grid_mask_row_words(A)
};
int64_t grid_mask_row_words(int A);
int launch_grid_mask(const GridMaskCall& c);

// ---- the applicability domain (grid_domain.hip; include/impnn.h, impnn_domain_grid / _grid_mask / _rows): the
// distance from a pair's latent vector mix_cat[i] + mix_an[j], or from a query row, to the nearest row of `ref` (R, Mx).
// api.hip checks the arguments.
struct DomainGridCall {
  const float *mix_cat, *mix_an, *ref;
  float* distance;   // (C, A); the materialising form
  int32_t* nearest;  // (C, A), or null
  uint32_t* words;   // (C, W); the mask form: distance and nearest null
  float lo, hi;
  int C, A, R, Mx;
  hipStream_t stream;
};
struct DomainRowsCall {
  const float *z, *ref;
  bool exclude_self;  // query p skips row p of the reference (Q == R)
  float* distance;    // (Q)
  int32_t* nearest;   // (Q), or null
  int Q, R, Mx;
  hipStream_t stream;
};
int domain_reference_chunk();  // reference rows per LDS chunk of the kernels
int launch_domain_grid(const DomainGridCall& c);
int launch_domain_rows(const DomainRowsCall& c);

// ---- the diverse batch (grid_diverse.hip; include/impnn.h, impnn_diverse_select): k pairs by farthest-point selection
// over the domain distance.  api.hip checks the arguments.
constexpr int kDiverseMaxK = 4096;  // picks per call: one launch each
struct DiverseCall {
  const float *mix_cat, *mix_an, *ref;
  const uint32_t* where;  // (C, W) mask words, or null: every pair
  int k;
  int32_t *cation, *anion;  // (k)
  float* distance;          // (k)
  int64_t* counts;          // (2): n, competing
  void* workspace;
  int C, A, R, Mx;
  hipStream_t stream;
};
size_t diverse_workspace_bytes(int C, int A, int k);
int launch_diverse_select(const DiverseCall& c);

// ---- the ensemble grid (ensemble_grid.hip; include/impnn.h, impnn_ensemble_grid*): family 2 of GridOperands through
// the materialising, mask-writing and selecting forms.  api.hip checks the arguments.
int ensemble_grid_max_members();
int ensemble_grid_max_temperatures(int kind, int M);  // a materialising or mask-writing launch; kind 1: 0
int ensemble_grid_topk_max_temperatures(int M);       // a selecting launch: 1 .. kSelectMaxT
int64_t ensemble_grid_tail_floats(int kind, int F, int Mx);
int launch_ensemble_grid(const GridOperands& g, float* mean, float* std, float* score);
int launch_ensemble_grid_mask(const GridMaskCall& c);
int launch_ensemble_grid_topk(const GridTopkCall& c);

// ---- Monte-Carlo dropout of the transfer head over the grid (transfer_mc_grid.hip; include/impnn.h,
// impnn_transfer_mc_grid*): family 3 of GridOperands through the materialising, mask-writing and selecting forms.
// api.hip checks the arguments.
int transfer_mc_grid_max_samples();
int launch_transfer_mc_grid(const GridOperands& g, float* mean, float* std, float* score, float* samples);
int launch_transfer_mc_grid_mask(const GridMaskCall& c);
int launch_transfer_mc_grid_topk(const GridTopkCall& c);

// ---- each ion's best partners over a cation x anion grid (grid_partners.hip; include/impnn.h,
// impnn_head_grid_partners / impnn_transfer_head_grid_partners).  The limits of one launch (ops.py mirrors them): m, at
// most kSelectMaxT temperatures, C * A < 2^32.
constexpr int kPartnersMaxM = 8;  // partners kept per ion: a tile column's running best lives in registers
// One partner-selecting launch: `where` may be null.  api.hip checks it.
struct GridPartnersCall {
  GridOperands g;
  const uint32_t* where;  // (C, ceil(A / 32)) words, or null: every pair competes
  int m, largest;
  float* cat_values;     // [max(nT,1)][C][m]
  int32_t* cat_partner;  // anion indices
  float* an_values;      // [max(nT,1)][A][m]
  int32_t* an_partner;   // cation indices
  void* workspace;
};
size_t grid_partners_workspace_bytes(int family, int C, int A, int nT, int m);
int launch_grid_partners(const GridPartnersCall& c);

// ---- the rank cut and the best-k pair mask over a cation x anion grid (grid_rank.hip; include/impnn.h,
// impnn_head_grid_rank / impnn_transfer_head_grid_rank): a radix select over the selection's 64-bit entries, most
// significant digit first, the grid evaluated once per digit (ops.py mirrors the digit width: RANK_DIGIT_BITS).
constexpr int kRankDigitBits = 8;
constexpr int kRankBins = 1 << kRankDigitBits;
constexpr int64_t kRankMaxPairs = ((int64_t)1 << 32) - 2;  // the entry format: a pair index stays below 2^32 - 1
// One call: `where` and `mask_words` may be null.  api.hip checks it.
struct GridRankCall {
  GridOperands g;
  int64_t k;
  int largest;
  const uint32_t* where;  // (C, ceil(A / 32)) words, or null: every pair competes
  float* values;          // [max(nT,1)]
  int32_t *cation, *anion;
  int64_t* count;
  uint32_t* mask_words;   // (C, W), viscosity (nT, C, W), or null: the rank cut alone
  void* workspace;
  int workgroups;
};
int grid_rank_passes(int64_t pairs);  // 4 key digits + the digits that hold pairs - 1
int grid_rank_workgroups(int family, int C, int A, int workgroups);  // 0: the default; capped by the tile count
size_t grid_rank_workspace_bytes(int family, int C, int A, int nT, int workgroups);
int launch_grid_rank(const GridRankCall& c);

// ---- per-ion statistics of a cation x anion grid (grid_summary.hip; include/impnn.h, impnn_*_grid_summary): every
// family of GridOperands through the summary form, then the merge of the tiles' partial records.
// One call: `where` may be null.  api.hip checks it.
struct GridSummaryCall {
  GridOperands g;
  const uint32_t* where;  // (C, ceil(A / 32)) words, or null: every pair competes
  int carry;              // 1: the anion records continue from what they hold
  uint32_t* cat_count;    // [planes][C]
  double* cat_sums;       // [planes][C][2]: s, q
  float* cat_range;       // [planes][C][2]: lo, hi
  uint32_t* an_count;     // [planes][A]
  double* an_sums;
  float* an_range;
  void* workspace;
};
int grid_summary_max_planes(int family, int M);  // planes one launch takes (family 2: with M members)
size_t grid_summary_workspace_bytes(int family, int C, int A, int planes);
int launch_grid_summary(const GridSummaryCall& c);

// ---- the typed-message family (message_typed.hip): edge sort by bond type, sorted forward, message adjoint
int64_t bmm_message_typed_bwd_workspace_ints(int B, int E, int Vb);
int launch_bmm_message_typed_sorted(const TypedMessageCall& c);  // a checked call (api.hip)
int launch_bmm_message_typed_bwd(const TypedMessageCall& c);     // a checked call (api.hip)

// ---- the small adjoints (layer_adjoints.hip): embedding, Reduce, pool
int launch_embed_gather_bwd(const int32_t* ids, const float* dout, float* dtable, int64_t rows, int vocab, int dim,
                            hipStream_t s);
// (embed_rows.hip) the listed rows' gradient, in one summation order and without float atomics
int launch_embed_rows_bwd(const int32_t* ids, const float* dout, const int32_t* row_list, int n_listed, float* dtable,
                          int64_t rows, int vocab, int dim, int accumulate, hipStream_t s);
int launch_reduce_scatter_bwd(const float* dagg, const int32_t* tgt, int tgt_stride, float* dm, int B, int N, int E,
                              int D, hipStream_t s);
int launch_global_sum_pool_bwd(const float* dp, const int32_t* ids, float* dh, int B, int N, int D, hipStream_t s);
// ---- bond-type matrices in training (bond_matrices_train.hip): the bond-table gradient, all layers in one launch
int launch_bond_type_matrices_bwd(const float* tb, const float* W, const float* dA, float* dW, float* dtb, int Vb,
                                  int K, int D, int accumulate, hipStream_t s);
int launch_bond_type_matrices_multi(const float* tb, const float* const* W, float* const* out, int n, int Vb, int K,
                                    int D, hipStream_t s);
int launch_bond_type_matrices_multi_bwd(const float* tb, const float* const* W, const float* const* dA,
                                        float* const* dW, float* dtb, int n, int Vb, int K, int D, int accumulate,
                                        hipStream_t s, float* workspace = nullptr);
int64_t bond_type_matrices_multi_bwd_workspace(int n, int Vb, int K, int D);
// ---- GatedUpdate backward (gated_update_bwd.hip), and the one-pass GEMM the bond-table gradient borrows for K >= 64
int launch_strided_gemm(const float* A, const float* B, float* out, int64_t rows, int M, int N, int64_t a_rs,
                        int64_t a_cs, int64_t b_rs, int64_t b_cs, hipStream_t s);
int64_t gated_update_param_floats(int D);
int64_t gated_update_bwd_workspace(int64_t rows, int D, bool row_list = false);
int launch_gated_update_bwd(const GatedUpdateCall& c);  // a checked call (api.hip)
// ---- optimizer (optimizer.hip): Adam, the learning-rate schedule
int launch_adam_clipnorm(const void* table, const void* sizes, int n_vars, int64_t step, int64_t* step_dev, float lr,
                         float b1, float b2, float eps, float clipnorm, hipStream_t s);
// The learning-rate record of impnn_adam_step_scheduled (include/impnn.h): word indices and schedule kinds.
enum : int {
  kLrKind = 0, kLrFlags = 1, kLrBase = 2, kLrParam = 3, kLrDecaySteps = 4, kLrWarmupSteps = 5, kLrTarget = 6,
  kLrBoundaryCount = 7, kLrBoundaries = 8, kLrValues = 16, kLrWords = 32, kLrMaxBoundaries = 8,
  kLrConstant = 0, kLrExponential = 1, kLrCosine = 2, kLrPiecewise = 3
};
int64_t adam_scheduled_workspace(int n_vars);
int launch_adam_scheduled(const void* table, const void* sizes, int n_vars, int64_t* step_dev, const void* record,
                          float b1, float b2, float eps, float clipnorm, float global_clipnorm, float weight_decay,
                          const int32_t* decay_flags, float* partials, hipStream_t s);
int launch_lr_schedule_eval(const void* record, const int64_t* steps, float* out, int n, hipStream_t s);
// ---- dropout counter and mask (dropout.hip)
int launch_dropout_step(int64_t* counter, int64_t* snapshot, hipStream_t s);
int launch_dropout_mask(const DropoutArgs& d, const int32_t* ridx, const int32_t* nrows_dev, int64_t max_rows, int D,
                        float* out, hipStream_t s);

// ---- batch assembly (loader_kernels.hip)
int launch_batch_assemble(int n_ions, const int32_t* sample_idx, int B, int M, const int32_t* const* atom_flat,
                          const int32_t* const* atom_off, const int32_t* const* edge_flat,
                          const int32_t* const* bond_flat, const int32_t* const* edge_off, int shift, int N, int L,
                          int32_t* const* atom_ids, int32_t* const* bond_ids, int32_t* const* conn,
                          const float* t_flat, float* t_out, hipStream_t s);

// ---- event-pair profiler (api.hip); record_* are no-ops unless enabled on this thread
void profile_record_start(hipStream_t s);
void profile_record_stop(hipStream_t s);

void* debug_stamp_buffer(size_t* bytes);  // thread-local diagnostics buffer (api.hip), usually null

// ---- fused encoders (encoder_fused.hip: pull form, modes 0/1; encoder_typed.hip: per-bond-type form, mode 2)
struct EncoderArgs {
  int n_ions;
  const int32_t* atom_ids[2];
  const int32_t* bond_ids[2];
  const int32_t* conn[2];
  const float* weights[2];   // canonical packed step weights (used when prepared[g] is null)
  const void* prepared[2];   // impnn_encoder_prepare_weights output for `mode`, or null
  int mode;                  // 0 f32, 1 f16x2, 2 f32 typed
  int phases;                // bit 0: plan kernels, bit 1: encoder kernel
  int nwg;                   // resolved persistent workgroups (encoder_workgroups), same for plan and run
  float* pooled[2];
  const float* atom_table;
  const float* bond_table;
  int Va, Vb, B, N, E, D, K, S;
  float ln_eps;
  void* workspace;
  size_t workspace_bytes;
};
bool encoder_fused_supported(int mode, int N, int E, int D, int K, int S, int Vb);
int encoder_workgroups(int n_ions, int B, int requested, int N, int E, int mode);
size_t encoder_fused_workspace_bytes(int mode, int n_ions, int B, int N, int E, int D, int S, int Vb, int nwg);
int launch_encoder_fused(const EncoderArgs& a, hipStream_t s);
int launch_encoder_phase(const EncoderArgs& a, hipStream_t s, bool plan_phase);
size_t encoder_prepared_bytes(int mode, int D, int S, int Vb);
int launch_encoder_prepare(const float* weights, const float* bond_table, int D, int K, int S, int Vb, int mode,
                           void* prepared, hipStream_t s);
// the same with the step-0 message table of the typed encoder (modes 2 / 3 at atom_dim 32) behind the image; every other
// mode and width: exactly the two above
size_t encoder_prepared_bytes_atoms(int mode, int D, int S, int Va, int Vb);
int launch_encoder_prepare_atoms(const float* weights, const float* bond_table, const float* atom_table, int Va, int D,
                                 int K, int S, int Vb, int mode, void* prepared, hipStream_t s);
// ... and with the step-0 gate table behind that (only where the message table is built)
size_t encoder_prepared_bytes_gates(int mode, int D, int S, int Va, int Vb);
int launch_encoder_prepare_gates(const float* weights, const float* bond_table, const float* atom_table, int Va, int D,
                                 int K, int S, int Vb, int mode, void* prepared, hipStream_t s);
int ensure_lds_limit(const void* kern, int slot);
int device_compute_units();  // CUs of the current device (cached per device index)
// Rows per workgroup of the wide (atom_dim 64 / 128) GatedUpdate forward / backward kernels: 64, or 16 below 8 K rows,
// where 64-row tiles cannot fill the chip (one definition: the launchers and the workspace sizing must agree).
inline int gu_wide_tile_rows(int64_t rows) { return rows < 8192 ? 16 : 64; }
// ---- wide states (encoder_wide.hip: atom_dim 64 / 128 behind the same entries, mode 2)
bool encoder_wide_supported(int N, int E, int D, int K, int S, int Vb);
size_t encoder_wide_workspace_bytes(int n_ions, int B, int N, int E, int D, int S, int Vb, bool x3);
bool encoder_wide_batch_covered(int n_ions, int B, int N, int E, int D, int Vb);  // 32-bit indices and row offsets hold
size_t encoder_wide_prepared_bytes(int D, int S, int Vb, bool x3);
int launch_encoder_wide_prepare(const float* weights, const float* bond_table, int D, int K, int S, int Vb, bool x3,
                                void* prepared, hipStream_t s);
int launch_encoder_wide(const EncoderArgs& a, hipStream_t s);

}  // namespace impnn
