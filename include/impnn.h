/*
 * impnn.h - C ABI of libimpnn.so: the MI355X (gfx950) implementation of the ionic-mpnn
 * message-passing forward path.
 *
 * The reference (goalheart/ionic-mpnn) is pure Python on TensorFlow/Keras and has no FFI of
 * its own; the interface replaced here is the set of TF ops each Keras layer's call() issues.
 * Every entry point cites the reference lines (relative to the reference root) it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), caller-allocated, row-major contiguous;
 *     float = IEEE fp32, ids / connectivity = int32 exactly as the reference's
 *     Input(dtype=tf.int32) tensors (train_viscosity.py:150-157);
 *   - B batch (one ion each), N padded atoms, E padded directed edge slots, D atom_dim,
 *     K bond_dim, S message-passing steps, Va/Vb vocabulary sizes including padding id 0;
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous enqueues that never
 *     allocate, free, synchronise or retain pointers past return (hipGraph-capturable);
 *   - return value: 0 = ok, negative = error (IMPNN_E_*); impnn_last_error_string() gives the
 *     thread-local text of the last failure.  No C++ exception crosses this boundary;
 *   - re-entrant: results depend on the arguments only.  The library's only mutable state is thread-local
 *     (last error text, the opt-in event profiler and debug stamp buffer of the calling thread) plus write-once
 *     per-device caches of device attributes;
 *   - indices are never trusted: an edge whose src or tgt is outside [0,N) is treated as a
 *     padding edge (contributes nothing), an embedding id outside [0,V) yields a zero row -
 *     the behaviour of TF's GPU gather/scatter kernels; tf-CPU's "raise" behaviour is
 *     available through impnn_validate_indices + the Python wrapper's debug mode.
 */
#ifndef IMPNN_H_
#define IMPNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMPNN_OK 0
#define IMPNN_E_BADARG (-1)      /* null pointer, non-positive size, misaligned buffer */
#define IMPNN_E_UNSUPPORTED (-2) /* shape outside what the kernel set covers */
#define IMPNN_E_LAUNCH (-3)      /* hipLaunch / hipGetLastError failure */
#define IMPNN_E_WORKSPACE (-4)   /* workspace too small */

typedef void* impnn_stream_t; /* hipStream_t */

/* library identity: returns IMPNN_ABI_VERSION */
#define IMPNN_ABI_VERSION 3
int impnn_abi_version(void);
/* text of the calling thread's last error ("" if none) */
const char* impnn_last_error_string(void);
/* name of the code object target the library was built for ("gfx950") */
const char* impnn_target_arch(void);

/* ---- a1/a2: keras Embedding lookup (train_viscosity.py:163-164,171-172;
 *      train_melting_point.py:149-150,157-158).  out[r,:] = table[ids[r],:], r < rows. */
int impnn_embed_gather(const int32_t* ids, const float* table, float* out, int64_t rows,
                       int32_t vocab, int32_t dim, impnn_stream_t stream);

/* ---- a4: BondMatrixMessage.call with a dense bond_state (models/layers.py:100-117).
 *      h (B,N,D), bond_state (B,E,K), conn (B,E,2)=[src,tgt], W=bond_transform (K,D,D)
 *      -> messages (B,E,D); rows with src==0 or tgt==0 are zero (models/layers.py:114-115). */
int impnn_bmm_message(const float* h, const float* bond_state, const int32_t* conn, const float* W,
                      float* messages, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                      impnn_stream_t stream);

/* ---- per-bond-type matrices (schedule A): A[v,i,j] = sum_k bond_table[v,k]*W[k,i,j].
 *      Equals tf.tensordot(bond_state, W) of models/layers.py:108 evaluated once per bond type
 *      instead of once per edge, valid because bond_state is always an Embedding lookup
 *      (train_viscosity.py:172, train_melting_point.py:158). out (Vb,D,D). */
int impnn_bond_type_matrices(const float* bond_table, const float* W, float* out, int32_t Vb,
                             int32_t K, int32_t D, impnn_stream_t stream);

/* ---- a4 from bond ids: messages[b,e,:] = A[bond_ids[b,e]] @ h[b,src[b,e],:], masked as a4. */
int impnn_bmm_message_typed(const float* h, const int32_t* bond_ids, const int32_t* conn,
                            const float* type_mats, float* messages, int32_t B, int32_t N,
                            int32_t E, int32_t D, int32_t Vb, impnn_stream_t stream);

/* ---- a5: Reduce.call (models/layers.py:57-83): agg[b,t,:] = sum_{e: tgt[b,e]=t, t>0} m[b,e,:],
 *      accumulated in edge-slot order (deterministic, == sequential scatter_nd on CPU).
 *      tgt is read as tgt[(b*E+e)*tgt_stride]: stride 1 for a contiguous (B,E) tensor, 2 to read
 *      conn[:,:,1] in place (pass conn+1), as the caller does at train_viscosity.py:182. */
int impnn_reduce_scatter_add(const float* messages, const int32_t* tgt, int32_t tgt_stride,
                             float* agg, int32_t B, int32_t N, int32_t E, int32_t D,
                             impnn_stream_t stream);

/* ---- a10: the orphan models/bond_matrix_message.py:37-65 signature: a4 then a5 in one launch,
 *      [h, bond_state, conn] -> agg (B,N,D).  W is (K,D*D) flat == (K,D,D) row-major. */
int impnn_bmm_fused(const float* h, const float* bond_state, const int32_t* conn, const float* W,
                    float* agg, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                    impnn_stream_t stream);

/* ---- a7: GatedUpdate (models/layers.py:142-156), forward and backward, one family of entries.
 *  Forward: GatedUpdate.call on `rows` = B*N atom rows (padding rows included, as the reference computes them).
 *  Wz/Wr/Wh are keras Dense kernels (2D,D) (input-major), b* (D,), LayerNormalization gamma/beta (D,), eps = 1e-3 by
 *  keras default.  Backward: dh, dagg (rows,D) and dparams, as "Backward" below describes.
 *
 *  entry (impnn_gated_update..)  rows         atom_dim              extra buffers              workspace query
 *  (forward)                     all          any                   -                          -
 *  _rows                         the list     32, 64, 128           row list                   -
 *  _rows_train                   list or all  32, 64, 128           row list or none, saved    -
 *  _dropout                      all          any                   dropout                    -
 *  _rows_train_dropout           list or all  any; with saved:      row list or none, saved    -
 *                                             32, 64, 128           or none, dropout
 *  _bwd                          all          divides 256           -                          _bwd_workspace_floats
 *  _rows_bwd                     the list     64, 128               row list                   _rows_bwd_workspace_floats
 *  _rows_bwd_saved               list or all  32 (all rows), 64,    row list or none, saved    _rows_bwd_...; at 32
 *                                             128                                              _bwd_workspace_floats
 *  _bwd_dropout, _rows_bwd_dropout, _rows_bwd_saved_dropout: the entry without the suffix, + dropout
 *
 *  Row list (row_index, n_rows): only rows row_index[0 .. *n_rows) of h / agg / out (dh / dagg) are read and written;
 *    the others are left untouched, and the parameter gradients are sums over the listed rows.  *n_rows lives on the
 *    device (no host round trip, capturable); the launch is sized for max_rows.  Padding atoms reach neither a message
 *    nor the pool (no valid edge names them), so a caller that owns the whole encode() loop may skip them:
 *    impnn_kept_rows and impnn_row_index_fill below build that list.  "row list or none": both NULL = all max_rows.
 *  saved (impnn_gated_update_rows_saved_floats(max_rows, D) = 4 D max_rows floats, 16-byte aligned): the training
 *    forward writes, per listed row (by list position), the gates z, r, the candidate tanh(.) and r * h of
 *    models/layers.py:145-152; the saving backward uses them instead of its two recompute GEMM passes (half of its
 *    matrix work) and CONSUMES the buffer (it comes back holding the pre-activation gradients; a second backward over
 *    it needs a second forward).
 *  dropout (rate, seed, step, layer_word) - Dropout(rate)(LN(n) + h, training=True) of models/layers.py:156, fused
 *    into the kernels.  The mask is not stored: element (row, column) of the (rows, D) output, row = the flat row of h
 *    (for row-list calls the row the list names, so both forms draw the same mask), draws word column % 4 of
 *        Philox4x32-10(counter = (column / 4, row, layer_word, lo32(*step)),
 *                      key     = (lo32(seed), hi32(seed) ^ hi32(*step)))
 *    and is kept iff (word >> 8) * 2^-24 >= rate; kept: out * (1.0f / (1.0f - rate)) (one f32 multiply), dropped: +0.
 *    layer_word = layer_id | (rank << 16).  `step` is a DEVICE int64 (a snapshot slot of impnn_dropout_step): the
 *    kernels read it when they run, so a captured step draws a fresh mask on every replay.  The forwards apply the
 *    mask on the final store (after the residual; `saved` keeps the pre-dropout values), the backwards read dout
 *    through the same mask and scale.
 *
 *  Rules shared by the family, checked in this order:
 *    1. dropout: step != NULL, then 0 <= rate < 1 (IMPNN_E_BADARG).  rate == 0 is the plain entry's call, results and
 *       status bit for bit (_rows_train_dropout: _rows_train with saved, else _rows with a row list, else the forward).
 *    2. rows >= 0 (IMPNN_E_BADARG); an atom_dim outside "any" (> 0) or "divides 256" is IMPNN_E_BADARG, outside a
 *       fixed set IMPNN_E_UNSUPPORTED, as is a saved buffer at an atom_dim other than 32, 64 and 128.
 *    3. the forwards: rows == 0 returns 0 before any pointer is read.
 *    4. a null tensor, or a row list with only one of row_index / n_rows: IMPNN_E_BADARG.
 *    5. then the forwards: saved 16-byte aligned, ln_eps >= 0 (IMPNN_E_BADARG); a row list at an atom_dim other
 *       than 32, 64 and 128 is IMPNN_E_UNSUPPORTED; at atom_dim 32 a row list or a saved buffer needs h, agg and out
 *       16-byte aligned (IMPNN_E_BADARG).
 *    6. then the backwards: a row list at an atom_dim other than 64 and 128 is IMPNN_E_UNSUPPORTED; workspace_floats
 *       below the form's query is IMPNN_E_WORKSPACE; rows == 0 then returns 0 for the row-list and saving forms (the
 *       plain backward still runs and writes dparams); the row-list and saving forms need h, agg, dout, dh, dagg,
 *       workspace and saved 16-byte aligned (IMPNN_E_BADARG).  The backwards do not check ln_eps. */
int impnn_gated_update(const float* h, const float* agg, const float* Wz, const float* bz,
                       const float* Wr, const float* br, const float* Wh, const float* bh,
                       const float* gamma, const float* beta, float ln_eps, float* out,
                       int64_t rows, int32_t D, impnn_stream_t stream);
int impnn_gated_update_rows(const float* h, const float* agg, const float* Wz, const float* bz,
                            const float* Wr, const float* br, const float* Wh, const float* bh,
                            const float* gamma, const float* beta, float ln_eps, float* out,
                            const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                            impnn_stream_t stream);
int64_t impnn_gated_update_rows_saved_floats(int64_t max_rows, int32_t D);
int impnn_gated_update_rows_train(const float* h, const float* agg, const float* Wz, const float* bz,
                                  const float* Wr, const float* br, const float* Wh, const float* bh,
                                  const float* gamma, const float* beta, float ln_eps, float* out,
                                  const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                  float* saved, impnn_stream_t stream);
int impnn_gated_update_dropout(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                               const float* br, const float* Wh, const float* bh, const float* gamma,
                               const float* beta, float ln_eps, float* out, int64_t rows, int32_t D, float rate,
                               uint64_t seed, const int64_t* step, int32_t layer_word, impnn_stream_t stream);
int impnn_gated_update_rows_train_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                          const float* Wr, const float* br, const float* Wh, const float* bh,
                                          const float* gamma, const float* beta, float ln_eps, float* out,
                                          const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                          float* saved, float rate, uint64_t seed, const int64_t* step,
                                          int32_t layer_word, impnn_stream_t stream);
int64_t impnn_gated_update_param_floats(int32_t D);
int64_t impnn_gated_update_bwd_workspace_floats(int64_t rows, int32_t D);
int impnn_gated_update_bwd(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                           const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                           const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                           int64_t workspace_floats, int64_t rows, int32_t D, int32_t accumulate,
                           impnn_stream_t stream);
int64_t impnn_gated_update_rows_bwd_workspace_floats(int64_t max_rows, int32_t D);
int impnn_gated_update_rows_bwd(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                                const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                                const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                                int64_t workspace_floats, const int32_t* row_index, const int32_t* n_rows,
                                int64_t max_rows, int32_t D, int32_t accumulate, impnn_stream_t stream);
int impnn_gated_update_rows_bwd_saved(const float* h, const float* agg, const float* Wz, const float* bz,
                                      const float* Wr, const float* br, const float* Wh, const float* bh,
                                      const float* gamma, float ln_eps, const float* dout, float* dh, float* dagg,
                                      float* dparams, float* workspace, int64_t workspace_floats,
                                      const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                      int32_t accumulate, float* saved, impnn_stream_t stream);
int impnn_gated_update_bwd_dropout(const float* h, const float* agg, const float* Wz, const float* bz, const float* Wr,
                                   const float* br, const float* Wh, const float* bh, const float* gamma, float ln_eps,
                                   const float* dout, float* dh, float* dagg, float* dparams, float* workspace,
                                   int64_t workspace_floats, int64_t rows, int32_t D, int32_t accumulate, float rate,
                                   uint64_t seed, const int64_t* step, int32_t layer_word, impnn_stream_t stream);
int impnn_gated_update_rows_bwd_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                        const float* Wr, const float* br, const float* Wh, const float* bh,
                                        const float* gamma, float ln_eps, const float* dout, float* dh, float* dagg,
                                        float* dparams, float* workspace, int64_t workspace_floats,
                                        const int32_t* row_index, const int32_t* n_rows, int64_t max_rows, int32_t D,
                                        int32_t accumulate, float rate, uint64_t seed, const int64_t* step,
                                        int32_t layer_word, impnn_stream_t stream);
int impnn_gated_update_rows_bwd_saved_dropout(const float* h, const float* agg, const float* Wz, const float* bz,
                                              const float* Wr, const float* br, const float* Wh, const float* bh,
                                              const float* gamma, float ln_eps, const float* dout, float* dh,
                                              float* dagg, float* dparams, float* workspace, int64_t workspace_floats,
                                              const int32_t* row_index, const int32_t* n_rows, int64_t max_rows,
                                              int32_t D, int32_t accumulate, float* saved, float rate, uint64_t seed,
                                              const int64_t* step, int32_t layer_word, impnn_stream_t stream);
/* The row list of an encode() loop: impnn_kept_rows gives, per molecule, r_b = 1 + max(last n with atom_ids[b,n] > 0,
 * largest atom index on a valid edge) (the kept rows are closed under "is a source of": skipping is exact), and
 * impnn_row_index_fill turns r and its inclusive prefix sum into the flat list b*N + [0, r_b) and its length (*n_rows,
 * device memory; the GatedUpdate launches are sized for max_rows = B*N). */
int impnn_kept_rows(const int32_t* atom_ids, const int32_t* bond_ids, const int32_t* conn, int32_t* rows_out,
                    int32_t B, int32_t N, int32_t E, int32_t Vb, impnn_stream_t stream);
int impnn_row_index_fill(const int32_t* kept_rows, const int32_t* kept_rows_inclusive_prefix,
                         int32_t* row_index, int32_t* n_rows, int32_t B, int32_t N, impnn_stream_t stream);

/* ---- a8: GlobalSumPool.call (models/layers.py:161-164): out[b,:] = sum_n h[b,n,:]*[ids[b,n]>0]. */
int impnn_global_sum_pool(const float* h, const int32_t* atom_ids, float* out, int32_t B,
                          int32_t N, int32_t D, impnn_stream_t stream);

/* ---- a9: encode() (train_viscosity.py:166-187; train_melting_point.py:152-171) up to and
 *      including GlobalSumPool, for `n_ions` independent ion branches in ONE launch
 *      (cation and anion: train_viscosity.py:193-194).
 *
 *  Per ion g < n_ions:  atom_ids[g] (B,N), bond_ids[g] (B,E), conn[g] (B,E,2), step weights
 *  weights[g] in the canonical packed layout below, pooled[g] (B,D).
 *  atom_table (Va,D) and bond_table (Vb,K) are shared by the ions (train_viscosity.py:163-164).
 *
 *  Canonical packed step-weight layout (floats), repeated S times per ion:
 *     bond_transform K*D*D | Wz 2D*D | bz D | Wr 2D*D | br D | Wh 2D*D | bh D | gamma D | beta D
 *  impnn_encoder_step_floats(D,K) returns that per-step count.
 *
 *  The arrays of pointers are HOST arrays of device pointers (length n_ions, n_ions <= 2). */
/*  `mode` - schedule and arithmetic of the encoder (an argument of every encoder entry; the library keeps no
 *  encoder state between calls):
 *    IMPNN_ENCODER_F32 (0):       "pull" form (agg = sum_k W_k G_k), v_mfma_f32_16x16x4_f32, exact f32 products;
 *                                 atom_dim 32, bond_dim <= 8.
 *    IMPNN_ENCODER_F16X2 (1):     pull form with each f32 operand split into two fp16 numbers, 3 fp16 MFMA products
 *                                 per f32 product, f32 accumulation (product error ~2^-21; narrower than f32).  Valid
 *                                 while |h|, |agg|, |G| < 4094 and |weights| < 255 - the caller's static bound
 *                                 (ionic_mpnn_amd.model checks it when weights are packed).
 *    IMPNN_ENCODER_F32_TYPED (2): per-bond-type form, the reference's own order of operations
 *                                 (models/layers.py:108-112): m_e = A[bond id of e] h[src_e] with
 *                                 A[v] = sum_k bond_table[v,k] W[k], on v_mfma_f32_4x4x1_16b_f32, exact f32 products;
 *                                 in-edge messages summed in edge-slot order.  atom_dim 32, ANY bond_dim (K = D^2 of
 *                                 train_melting_point.py:146 included), Vb <= 256, ANY padded shape N, E < 65536 (the
 *                                 explicit-hydrogen molecules of src/featurize.py:45 pad to E = 4 max_bonds,
 *                                 train_viscosity.py:288-289): one persistent kernel with the node state in LDS.  What
 *                                 bounds a molecule is what it HOLDS - kept rows <= 256, valid edges <= 512,
 *                                 in-degrees <= 255 - checked per batch by the plan kernels: a batch with a molecule
 *                                 beyond that gets NaN outputs and a nonzero int32 at byte
 *                                 impnn_encoder_plan_overflow_offset() of the workspace (device memory; a caller whose
 *                                 shapes allow it - N > 256 or E > 255 - reads the word back and takes the layer-at-a-
 *                                 time entries for that batch, as ionic_mpnn_amd.model does).  atom_dim 64 / 128 (train_viscosity.py with atom_dim=128,
 *                                 num_steps=6), N <= 256, E <= 1024, Vb <= 512: the same arithmetic as a short sequence
 *                                 of launches per call on compact kept rows (per type-run GEMMs for the messages,
 *                                 slot-order sums, GatedUpdate on 64-row tiles; csrc/encoder_wide.hip); `workgroups`
 *                                 is ignored there.  A batch must keep its compact rows within 32-bit float offsets,
 *                                 (n_ions B N + 128 n_ions + 128) D < 2^31 (52 427 pairs at N = 160, D = 128), and its
 *                                 edge slots within 32-bit indices: impnn_encoder_workspace_bytes answers
 *                                 IMPNN_E_UNSUPPORTED beyond that - split the batch.
 *    IMPNN_ENCODER_F32X3_TYPED (3): mode 2 with the GatedUpdate GEMMs on the bf16 matrix pipe: every f32 operand is carried
 *                                 EXACTLY as three bf16 terms (3 x 8 significant bits, fp32's exponent range) and all nine
 *                                 cross products are accumulated in f32 (9 x v_mfma_f32_16x16x32_bf16 per 8 f32 MFMAs):
 *                                 the products are the f32 products, only their summation order differs.  atom_dim 32:
 *                                 messages stay on the f32 4x4x1 MFMA; atom_dim 64 / 128: the per-type message GEMMs
 *                                 run the same way.  Same shapes as mode 2 (padded E > 512 included), same records,
 *                                 prepared buffer of its own (impnn_encoder_prepared_bytes with this mode).  Opt-in.
 *  `workgroups` - persistent workgroups of the launch: 0 = default (environment IMPNN_ENCODER_WORKGROUPS if set - a
 *  process-wide diagnostics override, read ONCE at the first call - else one per compute unit), n = min(max(n, 16), CUs);
 *  a multiple of that for very large batches or padded shapes (the size query, plan and run agree on it by themselves).  It fixes the workspace layout, so the size query, the plan and
 *  the run of one batch must agree - impnn_encoder_plan returns what it used in its plan info and impnn_encoder_run
 *  takes it from there.  Why it is a knob: a caller that keeps several batches in flight on several streams gets more
 *  out of the chip with fewer, longer-running workgroups per launch (bench.py --streams 3: 128). */
#define IMPNN_ENCODER_F32 0
#define IMPNN_ENCODER_F16X2 1
#define IMPNN_ENCODER_F32_TYPED 2
#define IMPNN_ENCODER_F32X3_TYPED 3
int64_t impnn_encoder_step_floats(int32_t D, int32_t K);
size_t impnn_encoder_plan_overflow_offset(void);
int impnn_encoder_workspace_bytes(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D,
                                  int32_t K, int32_t S, int32_t Vb, int32_t mode, int32_t workgroups,
                                  size_t* bytes);
/* Where the chunk plan of such a call lies in its workspace (atom_dim 32 only; other widths: IMPNN_E_UNSUPPORTED).  Same
 * arguments and refusals as impnn_encoder_workspace_bytes; launches nothing, writes nothing into a workspace.
 *   out = { nwg, max_sub, rows_off, vr_off, nsub_off, desc_off, ecap (0 for pull-form plans), plan_vmin }
 * nwg: persistent workgroups (`workgroups` resolved); max_sub: chunk slots per workgroup; byte offsets of int32 tables:
 * rows / vr [n_ions][B] (kept rows / virtual rows of every molecule), nsub [nwg] (chunks of a workgroup), desc
 * [nwg][max_sub][4] = {first molecule, molecules, valid edges (typed plans), virtual rows | ion << 16}; ecap: valid edges
 * a typed chunk holds; plan_vmin: the least virtual rows a molecule counts.  For tests and diagnostics: the layout is
 * not part of the ABI's promises beyond this query. */
int impnn_encoder_plan_layout(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                              int32_t S, int32_t Vb, int32_t mode, int32_t workgroups, int64_t out[8]);
/* Where the chunk records of such a call lie (typed modes 2 and 3 only; pull-form modes: IMPNN_E_UNSUPPORTED).  Same
 * arguments and refusals as impnn_encoder_plan_layout otherwise; launches nothing.
 *   out = { rec_off, rec_stride, grp_off, runs_off, nrun_off }
 * rec_off: byte offset of the records in the workspace, record (j, sl) of desc [nwg][max_sub] at rec_off +
 * (j * max_sub + sl) * rec_stride; inside a record: grp_off, the group table (16 bytes per group, the first word = bond
 * type | edges << 8), in run order; runs_off, the run table (u16: first group of every run, then the group count),
 * ordered by run length descending, then type, then piece; nrun_off, the run count (u16).  For tests and diagnostics. */
int impnn_encoder_plan_records(int32_t n_ions, int32_t B, int32_t N, int32_t E, int32_t D, int32_t K,
                               int32_t S, int32_t Vb, int32_t mode, int32_t workgroups, int64_t out[5]);
int impnn_encoder_fused(int32_t n_ions, const int32_t* const* atom_ids,
                        const int32_t* const* bond_ids, const int32_t* const* conn,
                        const float* atom_table, int32_t Va, const float* bond_table, int32_t Vb,
                        const float* const* weights, int32_t mode, float* const* pooled, int32_t B,
                        int32_t N, int32_t E, int32_t D, int32_t K, int32_t S, float ln_eps,
                        int32_t workgroups, void* workspace, size_t workspace_bytes,
                        impnn_stream_t stream);

/* ---- a9 with weights prepared once.  The kernel-side weight image (mode 0: transposed / padded f32; mode 1:
 *      pre-split fp16 hi/lo blocks; mode 2: the Vb per-bond-type matrices of every step in MFMA operand order plus
 *      the transposed GatedUpdate kernels) depends on the weights only, so a caller whose weights are fixed between
 *      calls (inference; every step of an epoch's evaluation) builds it once per ion and per mode and passes it to
 *      impnn_encoder_fused_prepared, which then launches only the two plan kernels and the encoder.
 *      impnn_encoder_fused (above) takes the canonical weights and rebuilds the image in the workspace on every call.
 *      `prepared`: device buffer of impnn_encoder_prepared_bytes(D, S, Vb, mode) bytes (0: shape not covered by the
 *      mode), 16B aligned;
 *      `bond_table` (Vb,K) is read by mode 2 only (may be NULL otherwise). */
size_t impnn_encoder_prepared_bytes(int32_t D, int32_t S, int32_t Vb, int32_t mode);
int impnn_encoder_prepare_weights(const float* weights, const float* bond_table, int32_t D, int32_t K,
                                  int32_t S, int32_t Vb, int32_t mode, void* prepared,
                                  size_t prepared_bytes, impnn_stream_t stream);
/* The same with the atom embedding table folded in (modes 2 / 3 at atom_dim 32, S >= 1).  In step 0 a source row holds
 * atom_table[atom id] - or zeros, for an id outside [0,Va) - so the step-0 message of an edge is one of Vb x (Va + 1)
 * vectors that depend on the weights only.  These entries append that table (128 B per entry) to the image, each entry
 * bit for bit what the encoder's message phase computes, and mark it in the image; the encoder then gathers step 0's
 * messages instead of multiplying them.  impnn_encoder_run / impnn_encoder_fused_prepared find the table by themselves
 * and use it only when Va, Vb and S of the launch are the image's - any other image, one from
 * impnn_encoder_prepare_weights included, runs as before, with the same results.  The table is built only while it stays
 * below 2 MiB (Vb * (Va + 1) * 128 B: half of one XCD's L2); beyond that, and for every other mode or atom_dim, the
 * size and the image are those of the two entries above.  The image must be rebuilt when atom_table changes.
 * `atom_table` (Va,D): 16B aligned. */
size_t impnn_encoder_prepared_bytes_atoms(int32_t D, int32_t S, int32_t Va, int32_t Vb, int32_t mode);
int impnn_encoder_prepare_weights_atoms(const float* weights, const float* bond_table, const float* atom_table,
                                        int32_t Va, int32_t D, int32_t K, int32_t S, int32_t Vb, int32_t mode,
                                        void* prepared, size_t prepared_bytes, impnn_stream_t stream);
/* The with-atoms image with a second table behind the first: in step 0 the accumulators of the gates z and r, after the
 * bias and W_h h and before W_agg agg, depend on (step 0's weights, atom id) only - Va + 1 rows of 64 floats (z 0..31,
 * r 0..31; row Va: a zero row), each bit for bit what the encoder's atom phase computes, so its step 0 loads them
 * instead of multiplying.  Built exactly where the message table is (same 2 MiB rule, modes 2 / 3, atom_dim 32, S >= 1):
 * the size is that of impnn_encoder_prepared_bytes_atoms plus (Va + 1) * 256 bytes, rounded up to 16, and without a
 * message table size and image are the with-atoms entries'.  The encoder uses the gate table only together with the
 * message table and only when the image says it is there: images of the entries above keep running as they did, with
 * the same results.  Same arguments, refusals and rebuild rule (atom_table, or any weight of step 0) as
 * impnn_encoder_prepare_weights_atoms. */
size_t impnn_encoder_prepared_bytes_gates(int32_t D, int32_t S, int32_t Va, int32_t Vb, int32_t mode);
int impnn_encoder_prepare_weights_gates(const float* weights, const float* bond_table, const float* atom_table,
                                        int32_t Va, int32_t D, int32_t K, int32_t S, int32_t Vb, int32_t mode,
                                        void* prepared, size_t prepared_bytes, impnn_stream_t stream);
int impnn_encoder_fused_prepared(int32_t n_ions, const int32_t* const* atom_ids,
                                 const int32_t* const* bond_ids, const int32_t* const* conn,
                                 const float* atom_table, int32_t Va, const float* bond_table,
                                 int32_t Vb, const void* const* prepared, int32_t mode,
                                 float* const* pooled, int32_t B, int32_t N, int32_t E, int32_t D,
                                 int32_t K, int32_t S, float ln_eps, int32_t workgroups, void* workspace,
                                 size_t workspace_bytes, impnn_stream_t stream);

/* ---- f1: everything after GlobalSumPool in one launch.
 *      kind 0 (viscosity, train_viscosity.py:189,197-214 + models/layers.py:10-49):
 *        fp_g = relu(pooled_g Wfp_g + bfp_g); mixed = relu(fp_cat Wp_cat + bp_cat) + relu(fp_an Wp_an + bp_an);
 *        [A,b,c] = mixed Wv + bv; out = A + clip(softplus(b),0,20) / (T/100 + clip(softplus(c),0.1,50) + 1e-6)
 *      kind 1 (melting point, train_melting_point.py:173,191-198): out = relu(mixed Wh + bh) Wo + bo
 *      head_weights (keras Dense kernels (in,out) then bias, in this order; impnn_model_head_floats):
 *        Wfp_cat D*F | bfp_cat F | Wfp_an | bfp_an | Wp_cat F*Mx | bp_cat Mx | Wp_an | bp_an |
 *        kind 0: Wv Mx*3 | bv 3        kind 1: Wh Mx*F | bh F | Wo F | bo 1
 *      pooled_* (B,D), temperature (B,1) in kelvin (kind 0 only), out (B,1).  D <= 128 (atom_dim of the encoder:
 *      train_viscosity.py's 32, or 128 for the wider models), F, Mx <= 64 (fp_size 32, mixing_size 20 in the reference). */
int64_t impnn_model_head_floats(int32_t kind, int32_t D, int32_t F, int32_t Mx);
int impnn_model_head(int32_t kind, const float* pooled_cat, const float* pooled_an,
                     const float* temperature, const float* head_weights, float* out, int32_t B,
                     int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- f1 over a Cartesian product: C cations x A anions (x nT temperatures) from C + A encoder rows.  An ion's branch
 *      meets its partner only at AddTwoTensors / Add, so the head splits in two (replaces train_viscosity.py:189,197-214
 *      and train_melting_point.py:173,191-198 evaluated on every pair of a screen).  Both entries read the packed
 *      head_weights of impnn_model_head (impnn_model_head_floats); D <= 128, F, Mx <= 64.
 *      impnn_head_ion_mix: ion 0 = cation, 1 = anion; pooled (M,D) ->
 *        mix[m,:] = relu(relu(pooled[m] Wfp_g + bfp_g) Wp_g + bp_g)   (M,Mx), the per-ion half of impnn_model_head.
 *      impnn_head_grid: mixed = mix_cat[i] + mix_an[j] (the cation term first), then the tail of impnn_model_head.
 *        kind 0: temperatures (nT) in kelvin, 1 <= nT <= 4096; out (C,A,nT) row-major; params NULL or (C,A,3), which
 *                receives the VFT parameters (A, B, C) of every pair (the reference's SliceParamA/B/C outputs).
 *        kind 1: out (C,A); temperatures and params NULL, nT 0.
 *      Element (i,j,t) has the bits impnn_model_head returns for the single sample (pooled_cat[i], pooled_an[j],
 *      T[t]): the same fmaf chains (bias first, inputs ascending), no atomics.  One difference, on non-finite input
 *      only: relu here keeps a NaN (as keras does), so a NaN pooled row gives NaN in exactly its row / column of the
 *      grid, where impnn_model_head's fmaxf turns it into 0.
 *      Checks in order: shape (sizes, limits, nT, kind, ion); zero work (M == 0, C == 0 or A == 0: IMPNN_OK, nothing
 *      touched); null pointers.  C * A * nT may exceed 2^31. */
int impnn_head_ion_mix(int32_t kind, int32_t ion, const float* pooled, const float* head_weights, float* mix,
                       int32_t M, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_head_grid(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                    const float* head_weights, float* out, float* params, int32_t C, int32_t A, int32_t nT,
                    int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- f1 for training (f4): the same head read from the INDIVIDUAL weight tensors - `weights` is a host array of
 *      device pointers in the order of impnn_model_head's packed layout (10 tensors for kind 0, 12 for kind 1), so a
 *      training step does not re-pack the head after every optimizer update - and its backward in one launch.
 *      impnn_model_head_bwd recomputes the forward per sample, writes dpooled_cat / dpooled_an (B,D) and ADDS the
 *      parameter gradients to dweights[i] (same order and shapes as weights[i]; float atomics, so the sum order
 *      over workgroups is not fixed - fp32 rounding-level run-to-run differences in these ~5k values).
 *      Gradient of clip follows tf.clip_by_value / torch.clamp: passes where min <= x <= max.
 *      D <= 128, F, Mx <= 64 (these entries and the loss entries below).  The backward keeps the weights and their
 *      gradient sums in LDS: it takes heads of at most impnn_model_head_bwd_max_floats() packed floats
 *      (impnn_model_head_floats rounded up to 4) and refuses wider ones with IMPNN_E_UNSUPPORTED.
 *      Replaces the autograd tape of train_viscosity.py:189-214 / train_melting_point.py:173-198. */
int64_t impnn_model_head_bwd_max_floats(void);
int impnn_model_head_tensors(int32_t kind, const float* pooled_cat, const float* pooled_an,
                             const float* temperature, const float* const* weights, float* out,
                             int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_model_head_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an,
                         const float* temperature, const float* const* weights, const float* dout,
                         float* dpooled_cat, float* dpooled_an, float* const* dweights, int32_t B,
                         int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- the head with the training loss folded in (train_viscosity.py:189,227-230):
 *        loss = mean_b (pred_b - y_b)^2 + sum_t l2[t] * sum(W_t^2)
 *      keras "mse" plus the kernel_regularizer=l2(...) penalties; `l2` is a HOST array with one lambda per weight tensor
 *      in the order of `weights` (0 for tensors without a penalty).  impnn_model_head_loss writes the scalar `loss`
 *      (device) and, when `pred` is not null, the predictions (B); the squared errors are summed per workgroup in
 *      sample order and by the last workgroup to arrive in workgroup order, so the value is reproducible.  `workspace`:
 *      impnn_model_head_loss_workspace_floats(B) floats, the first 4 bytes ZERO before the first call (every call
 *      leaves them zero); one workspace per stream in flight.
 *      impnn_model_head_loss_bwd: `dloss` is a device scalar (the gradient of the loss value, 1 for a plain
 *      loss.backward(), n_local/n_global on a data-parallel rank); the kernel forms 2 (pred_b - y_b) / B * dloss
 *      itself and adds 2 l2[t] W_t dloss to the parameter gradients once.  Replaces ~25 elementwise / reduction
 *      launches of the autograd tape per training step. */
int64_t impnn_model_head_loss_workspace_floats(int32_t B);
int impnn_model_head_loss(int32_t kind, const float* pooled_cat, const float* pooled_an,
                          const float* temperature, const float* const* weights, const float* l2,
                          const float* y, float* pred, float* loss, float* workspace,
                          int64_t workspace_floats, int32_t B, int32_t D, int32_t F, int32_t Mx,
                          impnn_stream_t stream);
int impnn_model_head_loss_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an,
                              const float* temperature, const float* const* weights, const float* l2,
                              const float* y, const float* dloss, float* dpooled_cat, float* dpooled_an,
                              float* const* dweights, int32_t B, int32_t D, int32_t F, int32_t Mx,
                              impnn_stream_t stream);

/* ---- the same with per-sample weights (keras model.fit(sample_weight=...), reduction sum_over_batch_size):
 *        loss = (1/B) * sum_b w_b * (pred_b - y_b)^2 + sum_t l2[t] * sum(W_t^2)
 *      B counts EVERY sample of the batch, those of weight 0 included - it is not sum_b w_b; the penalties are not
 *      weighted.  `sample_weight`: B device floats directly after `y`, 4-byte aligned, expected finite and >= 0 (the
 *      library does not read the values on the host; the Python layer checks them).  sample_weight == NULL is valid
 *      and IS the unweighted entry: impnn_model_head_loss[_bwd] are these entries with a null weight, and a null
 *      weight runs the kernels without any weight instruction, so the unweighted bits do not depend on this family.
 *      The backward's gradient seed per sample is w_b * 2 (pred_b - y_b) / B * dloss.  Same workspace
 *      (impnn_model_head_loss_workspace_floats), same launches, same fixed summation order, same status codes in the
 *      same order as the unweighted entries (a misaligned sample_weight: IMPNN_E_BADARG after the null pointers). */
int impnn_weighted_model_head_loss(int32_t kind, const float* pooled_cat, const float* pooled_an,
                                   const float* temperature, const float* const* weights, const float* l2,
                                   const float* y, const float* sample_weight, float* pred, float* loss,
                                   float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F,
                                   int32_t Mx, impnn_stream_t stream);
int impnn_weighted_model_head_loss_bwd(int32_t kind, const float* pooled_cat, const float* pooled_an,
                                       const float* temperature, const float* const* weights, const float* l2,
                                       const float* y, const float* sample_weight, const float* dloss,
                                       float* dpooled_cat, float* dpooled_an, float* const* dweights, int32_t B,
                                       int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- a9 in two halves, for callers that pipeline batches.  impnn_encoder_plan runs only the
 *      graph-dependent plan kernels (row counts, shares, chunk records) of a batch into `workspace`;
 *      impnn_encoder_run runs only the encoder kernel from a planned workspace.  The plan needs no
 *      weights, so a caller may plan batch i+1 (any stream) before or while batch i is encoded and
 *      order the two with events; every batch in flight needs its own workspace.
 *      impnn_encoder_plan fills `info` (host memory, plain data) with the shape, record kind and workgroup count
 *      it planned for; impnn_encoder_run takes its launch geometry from `info` and returns IMPNN_E_BADARG when its
 *      own shape arguments or the record kind of `mode` (modes 0/1 share one, modes 2/3 share the other) differ.  The
 *      workspace itself starts with the same facts (device side): an encoder kernel that finds a plan made for
 *      another geometry writes NaN to `pooled` instead of reading records at wrong offsets.
 *      impnn_encoder_fused_prepared(...) == impnn_encoder_plan(...) then impnn_encoder_run(...). */
typedef struct impnn_encoder_plan_info {
  int32_t v[12];
} impnn_encoder_plan_info;
int impnn_encoder_plan(int32_t n_ions, const int32_t* const* atom_ids, const int32_t* const* bond_ids,
                       const int32_t* const* conn, int32_t B, int32_t N, int32_t E, int32_t D,
                       int32_t K, int32_t S, int32_t Va, int32_t Vb, int32_t mode, int32_t workgroups,
                       void* workspace, size_t workspace_bytes, impnn_stream_t stream,
                       impnn_encoder_plan_info* info);
int impnn_encoder_run(int32_t n_ions, const int32_t* const* atom_ids, const float* atom_table,
                      int32_t Va, const float* bond_table, int32_t Vb, const void* const* prepared,
                      int32_t mode, float* const* pooled, int32_t B, int32_t N, int32_t E, int32_t D,
                      int32_t K, int32_t S, float ln_eps, const impnn_encoder_plan_info* info,
                      void* workspace, size_t workspace_bytes, impnn_stream_t stream);

/* ---- f2: batch assembly on the GPU - the step before the path.  Replaces, per batch, the host list
 *      handling of train_viscosity.py:291-314: np.array(list)[idx] of id lists shifted by +1
 *      (train_viscosity.py:255-262), pad_sequences_1d (utils/mp_utils.py:12-16) and
 *      preprocess_edges_and_bonds (utils/mp_utils.py:18-45: every (src,tgt) followed by (tgt,src) with
 *      the same bond id, then [0,0]/0 padding or truncation to L = 2*max_edges slots).
 *      The id dataset of M samples is flattened once, per ion g, into ragged device arrays:
 *        atom_flat[g] raw atom ids, atom_off[g] (M+1) offsets; edge_flat[g] (src,tgt) pairs and
 *        bond_flat[g] raw bond ids, both indexed by edge_off[g] (M+1) offsets (a sample's edge and bond
 *        lists are cut to the shorter of the two, as the reference's zip() does).
 *      For b < B and s = sample_idx[b]:
 *        atom_ids[g][b,:]  = atom_flat[g][sample s] + id_shift, right-padded with 0 to N;
 *        conn[g][b,2e,:]   = edge e, conn[g][b,2e+1,:] = its reverse (NOT shifted), bond_ids[g][b,2e..2e+1] =
 *        bond e + id_shift; slots >= min(2*n_edges, L) are 0;  t_out[b] = t_flat[s] (optional, may be NULL).
 *      A sample index outside [0,M) yields an all-padding sample; a sample with more than N atoms is cut
 *      at N (the reference raises on both: the Python wrapper checks them on the host).
 *      Pointer arrays are HOST arrays of device pointers; edge_flat / conn 8-byte aligned. */
int impnn_batch_assemble(int32_t n_ions, const int32_t* sample_idx, int32_t B, int32_t M,
                         const int32_t* const* atom_flat, const int32_t* const* atom_off,
                         const int32_t* const* edge_flat, const int32_t* const* bond_flat,
                         const int32_t* const* edge_off, int32_t id_shift, int32_t N, int32_t L,
                         int32_t* const* atom_ids, int32_t* const* bond_ids, int32_t* const* conn,
                         const float* t_flat, float* t_out, impnn_stream_t stream);

/* ---- the transfer head (train_melting_point_transfer.py:95-103): everything behind GlobalSumPool of the transfer model,
 *        pooled_cat, pooled_an -> fp Dense relu (per ion) -> proj Dense relu (per ion) -> add
 *          -> Dense 256 relu -> BatchNormalization -> Dense 128 relu -> Dropout -> Dense 64 relu -> Dense 1
 *      `weights` / `dweights`: HOST arrays of 18 device pointers (keras shapes, kernels (in,out)):
 *        Wfp_cat bfp_cat Wfp_an bfp_an Wp_cat bp_cat Wp_an bp_an W1 b1 gamma beta W2 b2 W3 b3 Wo bo
 *      moving_mean / moving_var (256): BatchNormalization's moving statistics.  D <= 128, F, Mx <= 64, any B >= 1.
 *      impnn_transfer_head: inference (moving statistics, no dropout), one launch, out (B,1).
 *      impnn_transfer_head_loss: loss = mean_b L(pred_b - y_b) + sum_t l2[t] * sum(W_t^2), L = e^2 (loss_kind 0) or
 *      Huber(delta) (loss_kind 1: e^2 / 2 for |e| <= delta, else delta (|e| - delta / 2)); `l2` a HOST array of 18
 *      lambdas.  bn_batch != 0 (a training pass of a trainable BatchNormalization): normalises with the batch mean and
 *      the biased batch variance and moves the moving statistics, moving -= (moving - batch) * (1 - bn_momentum), in
 *      device memory; three launches (the statistics sit between the two halves).  bn_batch == 0: the moving
 *      statistics, one launch.  rate > 0: Dropout behind the 128-wide Dense with the Philox mask of the
 *      GatedUpdate *_dropout entries on (row = sample, column = unit); rate == 0 ignores seed / step / layer_word.
 *      `saved` (impnn_transfer_head_saved_floats, may be null when bn_batch == 0): what the backward reads.
 *      `workspace`: impnn_transfer_head_loss_workspace_floats(B) floats, the first 4 bytes ZERO before the first call
 *      (every call leaves them zero).  `pred` (B) may be null.  All sums run in a fixed order: the same inputs give the
 *      same bits.
 *      impnn_transfer_head_loss_bwd: the same arguments as the forward of the pass plus `dloss` (device scalar);
 *      ADDS the parameter gradients to dweights[t] where that pointer is not null (a null entry is a frozen tensor:
 *      nothing is computed for it), 2 l2[t] W_t dloss included, and writes dpooled_cat / dpooled_an (B,D) unless both
 *      are null (a frozen encoder).  `workspace`: impnn_transfer_head_bwd_workspace_floats floats.  Three launches, four
 *      with bn_batch.
 *      Status codes: dropout first (rate > 0: step != NULL and rate < 1, IMPNN_E_BADARG), then shape, loss_kind and
 *      null pointers (IMPNN_E_BADARG), then the buffer sizes (IMPNN_E_WORKSPACE), then the widths
 *      (IMPNN_E_UNSUPPORTED). */
int64_t impnn_transfer_head_saved_floats(int32_t B, int32_t F, int32_t Mx);
int64_t impnn_transfer_head_bwd_workspace_floats(int32_t B, int32_t F, int32_t Mx);
int64_t impnn_transfer_head_loss_workspace_floats(int32_t B);
int impnn_transfer_head(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                        const float* moving_mean, const float* moving_var, float bn_eps, float* out, int32_t B,
                        int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_loss(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                             const float* l2, float* moving_mean, float* moving_var, float bn_momentum, float bn_eps,
                             int32_t bn_batch, const float* y, int32_t loss_kind, float delta, float rate,
                             uint64_t seed, const int64_t* step, int32_t layer_word, float* saved,
                             int64_t saved_floats, float* pred, float* loss, float* workspace,
                             int64_t workspace_floats, int32_t B, int32_t D, int32_t F, int32_t Mx,
                             impnn_stream_t stream);
int impnn_transfer_head_loss_bwd(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                 float* const* dweights, const float* l2, int32_t bn_batch, const float* y,
                                 int32_t loss_kind, float delta, const float* dloss, float rate, uint64_t seed,
                                 const int64_t* step, int32_t layer_word, const float* saved, int64_t saved_floats,
                                 float* workspace, int64_t workspace_floats, float* dpooled_cat, float* dpooled_an,
                                 int32_t B, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- the transfer head's loss with per-sample weights (keras sample_weight, reduction sum_over_batch_size):
 *        loss = (1/B) * sum_b w_b * L(pred_b - y_b) + sum_t l2[t] * sum(W_t^2),  L as above (squared error or Huber)
 *      B counts EVERY sample of the batch, those of weight 0 included - it is not sum_b w_b.  The weights touch the loss
 *      only: BatchNormalization's batch and moving statistics, the Dropout mask and the penalties are those of the
 *      unweighted pass.  `sample_weight`: B device floats directly after `y`, 4-byte aligned, expected finite and >= 0
 *      (values are not read on the host).  sample_weight == NULL is valid and IS the unweighted entry:
 *      impnn_transfer_head_loss[_bwd] are these entries with a null weight, and a null weight runs kernels without any
 *      weight instruction.  The backward's gradient seed per sample is w_b * L'(pred_b - y_b) / B * dloss.  Workspaces,
 *      launches, summation order and status codes as the unweighted entries (a misaligned sample_weight:
 *      IMPNN_E_BADARG after the null pointers). */
int impnn_weighted_transfer_head_loss(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                      const float* l2, float* moving_mean, float* moving_var, float bn_momentum,
                                      float bn_eps, int32_t bn_batch, const float* y, const float* sample_weight,
                                      int32_t loss_kind, float delta, float rate, uint64_t seed, const int64_t* step,
                                      int32_t layer_word, float* saved, int64_t saved_floats, float* pred, float* loss,
                                      float* workspace, int64_t workspace_floats, int32_t B, int32_t D, int32_t F,
                                      int32_t Mx, impnn_stream_t stream);
int impnn_weighted_transfer_head_loss_bwd(const float* pooled_cat, const float* pooled_an, const float* const* weights,
                                          float* const* dweights, const float* l2, int32_t bn_batch, const float* y,
                                          const float* sample_weight, int32_t loss_kind, float delta,
                                          const float* dloss, float rate, uint64_t seed, const int64_t* step,
                                          int32_t layer_word, const float* saved, int64_t saved_floats,
                                          float* workspace, int64_t workspace_floats, float* dpooled_cat,
                                          float* dpooled_an, int32_t B, int32_t D, int32_t F, int32_t Mx,
                                          impnn_stream_t stream);

/* ---- the transfer head's loss over indexed rows (stage 1 of transfer learning: a frozen encoder's pooled vectors are
 *      computed once per distinct ion and kept): sample b reads cat_table[cat_row[b]] (cat_table (C,D)) and
 *      an_table[an_row[b]] (an_table (A,D)) where the entries above read pooled_cat[b] / pooled_an[b]; no gathered
 *      (B,D) copy exists.  `cat_row` / `an_row`: B device int32 each, 4-byte aligned, expected in [0,C) / [0,A) (values
 *      are not read on the host; an index outside its table reads a row of zeros).  Everything behind the load is the
 *      code of the entries above - BatchNormalization with batch or moving statistics, the Dropout mask keyed on the
 *      sample's position in the batch, the loss and every sum's order - so the results have the bits of
 *      impnn_weighted_transfer_head_loss[_bwd] on the gathered rows.  `sample_weight` may be NULL (the unweighted
 *      loss).  The backward has no dpooled: a trainable encoder is the entries above.  Launches and workspaces as the
 *      entries above.  B == 0: IMPNN_OK, nothing touched.  Status codes in the order above; a null or misaligned index,
 *      or C < 1 / A < 1, is IMPNN_E_BADARG after the null pointers and the weights' alignment. */
int impnn_transfer_head_loss_rows(const float* cat_table, const float* an_table, const int32_t* cat_row,
                                  const int32_t* an_row, const float* const* weights, const float* l2,
                                  float* moving_mean, float* moving_var, float bn_momentum, float bn_eps,
                                  int32_t bn_batch, const float* y, const float* sample_weight, int32_t loss_kind,
                                  float delta, float rate, uint64_t seed, const int64_t* step, int32_t layer_word,
                                  float* saved, int64_t saved_floats, float* pred, float* loss, float* workspace,
                                  int64_t workspace_floats, int32_t B, int32_t C, int32_t A, int32_t D, int32_t F,
                                  int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_loss_rows_bwd(const float* cat_table, const float* an_table, const int32_t* cat_row,
                                      const int32_t* an_row, const float* const* weights, float* const* dweights,
                                      const float* l2, int32_t bn_batch, const float* y, const float* sample_weight,
                                      int32_t loss_kind, float delta, const float* dloss, float rate, uint64_t seed,
                                      const int64_t* step, int32_t layer_word, const float* saved,
                                      int64_t saved_floats, float* workspace, int64_t workspace_floats, int32_t B,
                                      int32_t C, int32_t A, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);

/* ---- the transfer head over a Cartesian product: C cations x A anions from C + A encoder rows, on the matrix cores.
 *      mix = relu(proj_cat) + relu(proj_an) is a sum and mp_dense_1 is linear in it before its relu, so
 *        a1[i,j] = relu(u_cat[i] + u_an[j]),  u_cat = mix_cat W1 (C,256),  u_an = mix_an W1 + b1 (A,256)
 *      (replaces train_melting_point_transfer.py:95-103 evaluated on every pair of a screen).  Inference semantics as
 *      impnn_transfer_head: moving statistics, no Dropout.  `weights`: the HOST array of 18 device pointers above.
 *      impnn_transfer_grid_prepare: W2, W3 in the operand order of v_mfma_f32_32x32x2_f32, BatchNormalization as
 *        scale = gamma / sqrt(moving_var + bn_eps), shift = beta - moving_mean * scale, then b2, b3, Wo, bo -> `image`
 *        (impnn_transfer_grid_image_floats() floats, 16B aligned).  Once per weight version; one small launch.
 *      impnn_transfer_ion_half: ion 0 = cation, 1 = anion; pooled (M,D) ->
 *        u[m,:] = relu(relu(pooled[m] Wfp_g + bfp_g) Wp_g + bp_g) W1 (+ b1 for the anion: the bias enters once)  (M,256).
 *      impnn_transfer_head_grid: out[i,j] = Dense1(relu(Dense64(relu(Dense128(bn(relu(u_cat[i] + u_an[j])))))))  (C,A)
 *        row-major; u_cat (C,256), u_an (A,256) and the image 16B aligned, `out` at any 4-byte alignment.  Exact f32
 *        products (a k-ordered fmaf chain per output); against impnn_transfer_head only the order of the sums and the
 *        factored first layer differ.  Element (i,j) depends on u_cat[i], u_an[j] and the image only - not on C, A, the
 *        position in the grid or the launch - and is reproducible bit for bit; no atomics.  relu keeps a NaN (as keras
 *        does), so a NaN u row gives NaN in exactly its row / column of the grid.
 *      Checks in order: shape (ion, sizes >= 0, widths > 0, bn_eps >= 0; IMPNN_E_BADARG); zero work (M == 0, C == 0 or
 *      A == 0: IMPNN_OK, nothing touched); null pointers, then alignment (IMPNN_E_BADARG) and image_floats below the
 *      query (IMPNN_E_WORKSPACE); the ranges D <= 128, F, Mx <= 64 (IMPNN_E_UNSUPPORTED).  C * A may exceed 2^31. */
int64_t impnn_transfer_grid_image_floats(void);
int impnn_transfer_grid_prepare(const float* const* weights, const float* moving_mean, const float* moving_var,
                                float bn_eps, float* image, int64_t image_floats, impnn_stream_t stream);
int impnn_transfer_ion_half(int32_t ion, const float* pooled, const float* const* weights, float* u, int32_t M,
                            int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_grid(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                             float* out, int32_t C, int32_t A, impnn_stream_t stream);

/* ---- the k best pairs of a screen, selected on the GPU: the grids above without their (C,A[,nT]) output.  The
 *      selecting kernels run the tile arithmetic of impnn_head_grid / impnn_transfer_head_grid (a selected value has the
 *      bits those entries write for the pair) in persistent workgroups and keep a running top k per temperature in LDS;
 *      a second small launch merges the workgroups' lists.  No C x A buffer, no float atomics, no global atomics.
 *      Order: a pair's entry is (key << 32) | (i * A + j), compared as an unsigned 64-bit integer.  key is the
 *      order-preserving integer image of the float (-0.0 < +0.0), complemented when `largest` != 0; every NaN has the
 *      key 0xFFFFFFFF in both directions.  So: by value, ties by cation then anion index, NaN last (by index), and
 *      the result is the exact top k under that order - independent of `workgroups` and of any schedule.
 *      Outputs, sorted: values (nT,k) float (a NaN comes back as the quiet NaN 0x7FC00000), cation (nT,k) and anion
 *      (nT,k) int32; the melting-point and transfer grids have one row (nT = 0 in the call).  With C * A < k only the
 *      first C * A slots of a row are pairs; the rest hold NaN / -1 / -1.
 *      Limits of one call: 1 <= k <= 1024; kind 0: 1 <= nT <= impnn_grid_topk_max_temperatures() (4; split longer
 *      sweeps, a row does not depend on the others); C * A < 2^32; the widths of impnn_head_grid.
 *      workgroups: 0 = the default (two per compute unit, at most one per tile); otherwise that many, at most one per
 *      tile.  workspace: impnn_grid_topk_workspace_bytes bytes for the same (family, C, A, nT, k, workgroups), 8-byte
 *      aligned, family 0 = impnn_head_grid_topk, 1 = impnn_transfer_head_grid_topk; it holds [workgroups][nT][k]
 *      entries between the two launches and carries nothing from call to call.
 *      impnn_transfer_head_grid_topk: u rows and image as impnn_transfer_head_grid (16B aligned).
 *      Checks in order: shape (kind, sizes, nT, k, the limits, C * A, workgroups >= 0; IMPNN_E_BADARG, a limit
 *      IMPNN_E_UNSUPPORTED); zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null pointers, then alignment and
 *      the image size; the workspace size (IMPNN_E_WORKSPACE).  No allocation, no synchronisation, no state. */
int32_t impnn_grid_topk_max_temperatures(void);
int impnn_grid_topk_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t k, int32_t workgroups,
                                    size_t* need);
int impnn_head_grid_topk(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, int32_t k, int32_t largest, float* values, int32_t* cation,
                         int32_t* anion, void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT,
                         int32_t D, int32_t F, int32_t Mx, int32_t workgroups, impnn_stream_t stream);
int impnn_transfer_head_grid_topk(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                  void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups,
                                  impnn_stream_t stream);

/* ---- a screen under a constraint: packed pair masks.  A mask over C cations x A anions is uint32_t words[C][W] with
 *      W = impnn_grid_mask_row_words(A) = ceil(A / 32); pair (i,j) is bit (j & 31) of words[i][j >> 5]; the pad bits
 *      (j >= A) are always 0.  Rows are word-aligned, and both grid kernels start a tile on a word boundary (64 and 32
 *      anions), so every word has one writer: no atomics, no pre-zeroing - a mask-writing call writes EVERY word of its
 *      output.  A viscosity mask is [nT][C][W], one plane per temperature.
 *      impnn_head_grid_mask / impnn_transfer_head_grid_mask: the arguments of impnn_head_grid (without params) /
 *        impnn_transfer_head_grid with (lo, hi, words) for `out`: bit (i,j[,t]) = lo <= v && v <= hi, where v has the
 *        bits the materialising entry writes for that element (the same tile arithmetic).  A NaN prediction fails both
 *        comparisons; lo = -inf or hi = +inf mean "no limit" on that side.  kind 0: 1 <= nT <= 4096; kind 1: nT 0 and
 *        temperatures NULL.  words 4-byte aligned.  No C x A float buffer exists.
 *        Checks in order: shape (kind, sizes, nT, widths > 0, image_floats >= 0, a NaN bound; IMPNN_E_BADARG); zero
 *        work (C == 0 or A == 0: IMPNN_OK, nothing touched); null pointers; alignment (IMPNN_E_BADARG) and the image
 *        size (IMPNN_E_WORKSPACE); the limits D <= 128, F, Mx <= 64, nT <= 4096 (IMPNN_E_UNSUPPORTED).  C * A may
 *        exceed 2^31.
 *      impnn_head_grid_topk_where / impnn_transfer_head_grid_topk_where: the plain entries above plus `where`, a
 *        (C,W) mask, 4-byte aligned, NULL is IMPNN_E_BADARG (a null-pointer rule); for viscosity the one mask applies to
 *        every temperature row.  The result is the exact top k, under the same 64-bit entry order, of the pairs whose
 *        bit is set; with fewer than k such pairs the remaining slots hold NaN / -1 / -1.  Limits, workspace
 *        (impnn_grid_topk_workspace_bytes serves both forms) and checks are the plain entries'.  A persistent workgroup
 *        passes over a tile (16 x 64, 8 x 32 pairs) none of whose bits is set before it loads a row, so a selective
 *        constraint costs about the tiles it leaves. */
int64_t impnn_grid_mask_row_words(int32_t A);
int impnn_head_grid_mask(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, float lo, float hi, uint32_t* words, int32_t C, int32_t A,
                         int32_t nT, int32_t D, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_grid_mask(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  float lo, float hi, uint32_t* words, int32_t C, int32_t A, impnn_stream_t stream);
int impnn_head_grid_topk_where(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                               const float* head_weights, const uint32_t* where, int32_t k, int32_t largest,
                               float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                               int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F, int32_t Mx, int32_t workgroups,
                               impnn_stream_t stream);
int impnn_transfer_head_grid_topk_where(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                        const uint32_t* where, int32_t k, int32_t largest, float* values,
                                        int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                                        int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream);

/* ---- each ion's best partners, selected on the GPU: for every cation its m best anions and for every anion its m
 *      best cations, from ONE launch over the grid and without its (C,A[,nT]) output.  The partner-selecting kernels run
 *      the tile arithmetic of impnn_head_grid / impnn_transfer_head_grid (a selected value has the bits those entries
 *      write for the pair), one tile (16 x 64, 8 x 32 pairs) per workgroup, and select from the tile's values on the
 *      chip: a tile row by m rounds of a 64-bit minimum across a wave's lanes, a tile column by one thread that keeps m
 *      entries in registers; a second small launch, one thread per (temperature, ion), merges the tiles' candidates.
 *      No C x A buffer, no atomics, no pre-zeroed memory.
 *      Order: the entry of impnn_head_grid_topk, (key << 32) | (i * A + j), compared as an unsigned 64-bit integer.  For
 *      a fixed cation that is: by value, ties by anion index, NaN last; for a fixed anion: by value, ties by cation
 *      index, NaN last.  The result is exact and independent of tiles, launches and schedule.
 *      where: NULL, or a (C,W) pair mask (see below), 4-byte aligned: only pairs whose bit is set compete, the one mask
 *      for every temperature; a workgroup passes over a tile none of whose bits is set before it loads a row.
 *      Outputs: cat_values float / cat_partner int32 [max(nT,1)][C][m], the anion index of cation i's s-th best in
 *      slot [t][i][s]; an_values / an_partner [max(nT,1)][A][m], cation indices.  Ascending under the order; a NaN
 *      value comes back as the quiet NaN 0x7FC00000; slots past the number of competing partners of that ion hold
 *      NaN / -1.  The melting-point and transfer grids have one plane (nT = 0 in the call).
 *      Limits of one call: 1 <= m <= 8; kind 0: 1 <= nT <= 4 (split longer sweeps, a plane does not depend on the
 *      others); C * A < 2^32; the widths of impnn_head_grid.
 *      workspace: impnn_grid_partners_workspace_bytes bytes for the same (family, C, A, nT, m), 8-byte aligned, family
 *      0 = impnn_head_grid_partners, 1 = impnn_transfer_head_grid_partners; it holds [nT][tiles_a][C][m] and
 *      [nT][tiles_c][A][m] entries between the two launches, every one written by the first, and carries nothing from
 *      call to call.
 *      Checks in order, as impnn_head_grid_topk: shape (kind, sizes, nT, m, the limits, C * A; IMPNN_E_BADARG, a limit
 *      IMPNN_E_UNSUPPORTED); zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null pointers, then alignment and
 *      the image size; the workspace size (IMPNN_E_WORKSPACE).  No allocation, no synchronisation, no state. */
int impnn_grid_partners_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t m, size_t* need);
int impnn_head_grid_partners(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                             const float* head_weights, const uint32_t* where, int32_t m, int32_t largest,
                             float* cat_values, int32_t* cat_partner, float* an_values, int32_t* an_partner,
                             void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t D,
                             int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_grid_partners(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                      const uint32_t* where, int32_t m, int32_t largest, float* cat_values,
                                      int32_t* cat_partner, float* an_values, int32_t* an_partner, void* workspace,
                                      size_t workspace_bytes, int32_t C, int32_t A, impnn_stream_t stream);

/* ---- the rank cut and the best-k pair mask, by radix select on the GPU: for every temperature plane the k-th entry
 *      (1-based) of the order of impnn_head_grid_topk - (key << 32) | (i * A + j), compared as an unsigned 64-bit
 *      integer: by value, ties by cation then anion index, NaN last, `largest` complementing the key - and, optionally,
 *      the pairs at or before it as a packed pair mask.  k is not limited by on-chip memory: the k-th entry is found one
 *      8-bit digit a pass (impnn_grid_rank_digit_bits), most significant first, four passes over the key and one per
 *      byte that C * A - 1 needs (impnn_grid_rank_passes: 4 .. 8).  A pass runs the tile arithmetic of impnn_head_grid /
 *      impnn_transfer_head_grid (an entry has the bits those entries write for its pair) in persistent workgroups,
 *      counts the entries that share the digits found so far by their next digit in LDS, and a one-workgroup-per-plane
 *      step launch takes the digit; the state stays in the workspace, and a call enqueues every launch without a host
 *      round trip.  No C x A buffer, no global atomics, no float atomics, no pre-zeroed memory; the result is exact and
 *      does not depend on `workgroups` or the schedule.
 *      where: NULL, or a (C,W) pair mask, 4-byte aligned: only pairs whose bit is set compete, the one mask for every
 *      plane; a workgroup passes over a tile none of whose bits is set before it loads a row.
 *      Outputs, [max(nT,1)] each: values float, cation / anion int32 of the k-th entry (a NaN value comes back as the
 *      quiet NaN 0x7FC00000), count int64 (8-byte aligned) the number of competing pairs.  k > count: NaN / -1 / -1.
 *      mask_words: NULL, or (C,W) words, kind 0 (nT,C,W), 4-byte aligned, every one written: bit (i, j[, t]) is set
 *      for exactly the first min(k, count) competing pairs of plane t (a run of equal values that straddles k is cut by
 *      index), pad bits 0.
 *      Limits of one call: C * A <= 2^32 - 2; kind 0: 1 <= nT <= 4; the widths of impnn_head_grid.  workgroups: 0 for the
 *      default (one per compute unit), capped by the tile count.
 *      workspace: impnn_grid_rank_workspace_bytes bytes for the same (family, C, A, nT, workgroups), 8-byte aligned,
 *      family 0 = impnn_head_grid_rank, 1 = impnn_transfer_head_grid_rank; it carries nothing from call to call.
 *      Checks in order, one text each: kind; shape; zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null
 *      pointers, then alignment and the image size; k < 1; the pair count; nT; the workspace size (IMPNN_E_WORKSPACE);
 *      the widths (IMPNN_E_UNSUPPORTED, as the limits).  No allocation, no synchronisation, no state. */
int32_t impnn_grid_rank_digit_bits(void);
int32_t impnn_grid_rank_passes(int32_t C, int32_t A);
int impnn_grid_rank_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t nT, int32_t workgroups, size_t* need);
int impnn_head_grid_rank(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                         const float* head_weights, int64_t k, int32_t largest, const uint32_t* where, float* values,
                         int32_t* cation, int32_t* anion, int64_t* count, uint32_t* mask_words, void* workspace,
                         size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F, int32_t Mx,
                         int32_t workgroups, impnn_stream_t stream);
int impnn_transfer_head_grid_rank(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                  int64_t k, int32_t largest, const uint32_t* where, float* values, int32_t* cation,
                                  int32_t* anion, int64_t* count, uint32_t* mask_words, void* workspace,
                                  size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream);

/* ---- a deep ensemble over the grid: M members of one kind (0 viscosity, 1 melting point), trained from different
 *      seeds or folds, evaluated inside one grid tile, and per element the mean, the spread and a confidence-bound score
 *      of their M predictions - the third grid family, through the materialising, the mask-writing and the selecting
 *      form.  An ensemble screen is one launch over the grid; M grids never exist.
 *      Operands: mix_cat (M,C,Mx) and mix_an (M,A,Mx), member m's impnn_head_ion_mix rows (from its own encoder and
 *      its own per-ion weights; D does not reach the grid); temperatures as impnn_head_grid; tails (M, tail_floats),
 *      member m's tail section of impnn_model_head's packed layout, impnn_ensemble_grid_tail_floats(kind, F, Mx) floats:
 *      kind 0 Wv Mx*3 | bv 3; kind 1 Wh Mx*F | bh F | Wo F | bo 1.  F, Mx <= 64 and equal for all members.
 *      The statistic, in float32 and in this order, of the member values v_0 .. v_{M-1} of one element, where v_m has
 *      the bits impnn_head_grid gives member m for the same mixing rows:
 *        s = v_0; s = s + v_m, m ascending; mean = s / (float)M
 *        q = 0; d = v_m - mean; q = fmaf(d, d, q), m ascending; std = sqrt(q / (float)M)   (population, as numpy.std)
 *        score = fmaf(kappa, std, mean)                              kappa: any finite float
 *      with the correctly rounded division and square root, no atomics, every sum in a fixed order: an element's bits
 *      do not depend on the grid's size, the host tiling or the entry that produced it.  A NaN member value makes
 *      mean, std and score NaN for that element and for no other.  M = 1: mean = v_0, std = 0, score = mean.
 *      Limits: 1 <= M <= impnn_ensemble_grid_max_members() (8); kind 0: 1 <= nT <=
 *      impnn_ensemble_grid_max_temperatures(kind, M) for the materialising and the mask-writing entry (4096 for every M;
 *      0 for kind 1, which takes none) and <= impnn_ensemble_grid_topk_max_temperatures(M) for the selecting entries
 *      (4 up to M = 6, 3 at M = 7, 2 at M = 8: the members' kept results share the LDS with the lists; split longer
 *      sweeps, a row does not depend on the others).  The three functions return 0 for an M out of range,
 *      impnn_ensemble_grid_tail_floats -1 for a bad argument.
 *      impnn_ensemble_grid: mean, std, score (C,A,nT) for kind 0, (C,A) for kind 1, row-major; a NULL one is not
 *        written, at least one is needed.  Checks in order: kind; shape (sizes, nT for the kind; IMPNN_E_BADARG); M
 *        (below 1 IMPNN_E_BADARG, above the limit IMPNN_E_UNSUPPORTED) and kappa (NaN or infinite: IMPNN_E_BADARG); the
 *        limits F, Mx <= 64 and nT (IMPNN_E_UNSUPPORTED); zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null
 *        pointers; kind 1 with temperatures.  C * A * nT may exceed 2^31.
 *      impnn_ensemble_grid_mask: words as impnn_head_grid_mask, bit (i,j[,t]) = lo <= score && score <= hi.  Checks in
 *        order: kind; shape; M and kappa; a NaN bound; zero work; null pointers; alignment; the limits.
 *      impnn_ensemble_grid_topk / _topk_where: outputs, order, k <= 1024, C * A < 2^32, workgroups and `where` as
 *        impnn_head_grid_topk / _topk_where, on the score; workspace: impnn_ensemble_grid_topk_workspace_bytes bytes for
 *        the same (M, C, A, nT, k, workgroups), 8-byte aligned (impnn_grid_topk_workspace_bytes does not serve this
 *        family).  Checks in order: kind; shape; M and kappa; k, nT, C * A (the limits IMPNN_E_UNSUPPORTED); the
 *        widths; zero work; null pointers, then alignment; the workspace size (IMPNN_E_WORKSPACE).
 *      Each ion's best partners and the rank cut are not built for this family. */
int32_t impnn_ensemble_grid_max_members(void);
int32_t impnn_ensemble_grid_max_temperatures(int32_t kind, int32_t M);
int32_t impnn_ensemble_grid_topk_max_temperatures(int32_t M);
int64_t impnn_ensemble_grid_tail_floats(int32_t kind, int32_t F, int32_t Mx);
int impnn_ensemble_grid(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an, const float* temperatures,
                        const float* tails, float kappa, float* mean, float* std, float* score, int32_t C, int32_t A,
                        int32_t nT, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_ensemble_grid_mask(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                             const float* temperatures, const float* tails, float kappa, float lo, float hi,
                             uint32_t* words, int32_t C, int32_t A, int32_t nT, int32_t F, int32_t Mx,
                             impnn_stream_t stream);
int impnn_ensemble_grid_topk_workspace_bytes(int32_t M, int32_t C, int32_t A, int32_t nT, int32_t k, int32_t workgroups,
                                             size_t* need);
int impnn_ensemble_grid_topk(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                             const float* temperatures, const float* tails, float kappa, int32_t k, int32_t largest,
                             float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                             int32_t C, int32_t A, int32_t nT, int32_t F, int32_t Mx, int32_t workgroups,
                             impnn_stream_t stream);
int impnn_ensemble_grid_topk_where(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                                   const float* temperatures, const float* tails, float kappa, const uint32_t* where,
                                   int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                   void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t nT, int32_t F,
                                   int32_t Mx, int32_t workgroups, impnn_stream_t stream);

/* ---- Monte-Carlo dropout of the transfer head over the grid: S stochastic passes of one trained transfer model, with
 *      the head's Dropout (between Dense 128 and Dense 64) on and BatchNormalization on its moving statistics, evaluated
 *      inside one grid tile, and per pair the mean, the spread and a confidence-bound score of the S values - the fourth
 *      grid family, through the materialising, the mask-writing and the selecting form.
 *      Operands: u_cat, u_an, image, image_floats as impnn_transfer_head_grid; multipliers (S,128) float32, 16-byte
 *      aligned: sample s multiplies feature j of relu(Dense 128) by multipliers[s][j] - a feature whose multiplier is 0
 *      is 0 (also where the activation is not finite), any other is relu(a2)[j] * multipliers[s][j].  Then Dense 64,
 *      relu and Dense 1 exactly as impnn_transfer_head_grid: with every multiplier 1 a sample has that entry's bits.
 *      impnn_dropout_mask(seed, step, layer word, rate, NULL, NULL, S, 128, ...) writes the table of a Dropout: row s
 *      is the mask a training pass at that step applies to batch row s.  No generator runs inside the grid kernel.
 *      The table is the same for every pair of the grid (the "fixed set of masks" form of MC dropout): a pair's S
 *      values, and so its statistic, depend on its two u rows, the image and the table only, not on the tile, the
 *      launch, the host tiling or the grid's size.
 *      The statistic of a pair's values v_0 .. v_{S-1}, in float32 and in this order (impnn_ensemble_grid's, for S):
 *        s = v_0; s = s + v_i, i ascending; mean = s / (float)S
 *        q = 0; d = v_i - mean; q = fmaf(d, d, q), i ascending; std = sqrt(q / (float)S)   (population, as numpy.std)
 *        score = fmaf(kappa, std, mean)                              kappa: any finite float
 *      A NaN sample makes mean, std and score NaN for that pair and for no other.  S = 1: std = 0, score = mean.
 *      Limit: 1 <= S <= impnn_transfer_mc_grid_max_samples() (64: the samples' values and the table share a compute
 *      unit's LDS with the selecting form's list and mask words).
 *      impnn_transfer_mc_grid: mean, std, score (C,A) and samples (S,C,A), row-major; a NULL one is not written, at
 *        least one is needed.  Checks in order: shape (IMPNN_E_BADARG); S (below 1 IMPNN_E_BADARG, above the limit
 *        IMPNN_E_UNSUPPORTED) and kappa (NaN or infinite: IMPNN_E_BADARG); zero work (C == 0 or A == 0: IMPNN_OK, nothing
 *        touched); null pointers; alignment, then the image size (IMPNN_E_WORKSPACE).
 *      impnn_transfer_mc_grid_mask: words as impnn_transfer_head_grid_mask, bit (i,j) = lo <= score && score <= hi.
 *        Checks in order: shape; S and kappa; a NaN bound; zero work; null pointers; alignment and the image size.
 *      impnn_transfer_mc_grid_topk / _topk_where: outputs (1,k), order, k <= 1024, C * A < 2^32, workgroups and `where`
 *        as impnn_transfer_head_grid_topk / _topk_where, on the score; workspace:
 *        impnn_transfer_mc_grid_topk_workspace_bytes bytes for the same (S, C, A, k, workgroups), 8-byte aligned.  Checks
 *        in order: shape; S and kappa; k, C * A (the limits IMPNN_E_UNSUPPORTED); zero work; null pointers, then
 *        alignment and the image size; the workspace size (IMPNN_E_WORKSPACE).
 *      Each ion's best partners, the rank cut and Pareto objectives are not built for this family. */
int32_t impnn_transfer_mc_grid_max_samples(void);
int impnn_transfer_mc_grid(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                           const float* multipliers, int32_t S, float kappa, float* mean, float* std, float* score,
                           float* samples, int32_t C, int32_t A, impnn_stream_t stream);
int impnn_transfer_mc_grid_mask(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                const float* multipliers, int32_t S, float kappa, float lo, float hi, uint32_t* words,
                                int32_t C, int32_t A, impnn_stream_t stream);
int impnn_transfer_mc_grid_topk_workspace_bytes(int32_t S, int32_t C, int32_t A, int32_t k, int32_t workgroups,
                                                size_t* need);
int impnn_transfer_mc_grid_topk(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                const float* multipliers, int32_t S, float kappa, int32_t k, int32_t largest,
                                float* values, int32_t* cation, int32_t* anion, void* workspace, size_t workspace_bytes,
                                int32_t C, int32_t A, int32_t workgroups, impnn_stream_t stream);
int impnn_transfer_mc_grid_topk_where(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                      const float* multipliers, int32_t S, float kappa, const uint32_t* where,
                                      int32_t k, int32_t largest, float* values, int32_t* cation, int32_t* anion,
                                      void* workspace, size_t workspace_bytes, int32_t C, int32_t A, int32_t workgroups,
                                      impnn_stream_t stream);

/* ---- per-ion statistics of the grid, reduced on the GPU: for every cation over its anions, and for every anion over its
 *      cations, the number of competing pairs, the sum, the sum of squares, the least and the greatest value - the
 *      main-effects view of the cation x anion table, from ONE launch over the grid and without its (C,A[,nT]) output.
 *      The sixth operation of the screening family and the one every grid family has: the ensemble grid and the transfer
 *      MC grid summarise their score mean + kappa * std.
 *      The summary kernels run the tile arithmetic of the family's materialising entry (a summarised value v has the bits
 *      that entry writes for the pair), one tile (16 x 64 pairs; the transfer grids 8 x 32) per workgroup, and reduce the
 *      tile on the chip; a second small launch, one thread per (plane, ion), adds the tiles' partial records.  No C x A
 *      buffer, no atomics, no pre-zeroed memory.
 *      A pair competes when its `where` bit is set (NULL: always) and v is not NaN.  The record of an ion and plane:
 *        n: uint32, the competing pairs;  s = sum (double)v;  q = sum (double)v * (double)v (exact products);
 *        lo, hi: the least and the greatest v under the order of impnn_head_grid_topk's key (-0.0 < +0.0);
 *        n == 0: s = q = +0.0, lo = hi = the quiet NaN 0x7FC00000.
 *      The sums run in double in one order, a pair that does not compete being +0.0; (bc, ba) = the tile, (16, 64) or
 *      (8, 32).  Cation i: the anions in blocks of ba from anion 0, a block's partial the adjacent-pair tree
 *      x[2k] + x[2k+1] level by level, the total +0.0 plus the blocks in ascending order.  Anion j: the cations in blocks
 *      of bc from cation 0, a block's partial +0.0 plus its cations in ascending order, the total +0.0 (carry == 1: the
 *      record the buffers hold) plus the blocks in ascending order.  A tile the mask lets a workgroup pass over gives the
 *      partials computing it would give.  So the bits do not depend on the grid's size, on whether a masked-out tile was
 *      skipped, or - when a caller cuts the cation axis at multiples of 16 and carries the anion records from one range's
 *      call into the next - on that cut.
 *      where: NULL, or a (C,W) pair mask, 4-byte aligned, the one mask for every plane.
 *      carry: 0, the anion records are written without being read; 1, they continue from what they hold.
 *      buffers: a HOST table of seven device pointers, planes = max(nT, 1): cat_count uint32 [planes][C], cat_sums double
 *      [planes][C][2] (s, q; 8-byte aligned), cat_range float [planes][C][2] (lo, hi), an_count [planes][A], an_sums
 *      [planes][A][2], an_range [planes][A][2], and the workspace (8-byte aligned): workspace_bytes >=
 *      impnn_grid_summary_workspace_bytes(family, C, A, planes) = 32 * planes * (tiles_a * C + tiles_c * A) bytes, family
 *      0 head, 1 transfer, 2 ensemble, 3 transfer MC grid; the query answers 0 for arguments no launch takes.  The
 *      workspace is written before it is read and carries nothing from call to call.
 *      Limits of one call: nT <= 4096 (kind 0); the widths, M, S and kappa of the family's other entries.
 *      The ensemble grid's entry is impnn_deep_ensemble_grid_summary: the names that begin impnn_ensemble_grid are the
 *      closed list of that family's materialising, mask-writing and selecting entries and their queries.
 *      Checks in order, as impnn_head_grid_partners: kind and shape (with M or S and kappa, carry; IMPNN_E_BADARG, a
 *      limit IMPNN_E_UNSUPPORTED); the widths; zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null pointers
 *      (the table and each of its seven entries), then alignment and the image size; the workspace size
 *      (IMPNN_E_WORKSPACE, nothing touched).  No allocation, no synchronisation, no state. */
int64_t impnn_grid_summary_workspace_bytes(int32_t family, int32_t C, int32_t A, int32_t planes);
int impnn_head_grid_summary(int32_t kind, const float* mix_cat, const float* mix_an, const float* temperatures,
                            const float* head_weights, const uint32_t* where, int32_t carry, size_t workspace_bytes,
                            const void* const* buffers, int32_t C, int32_t A, int32_t nT, int32_t D, int32_t F,
                            int32_t Mx, impnn_stream_t stream);
int impnn_transfer_head_grid_summary(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                     const uint32_t* where, int32_t carry, size_t workspace_bytes,
                                     const void* const* buffers, int32_t C, int32_t A, impnn_stream_t stream);
int impnn_deep_ensemble_grid_summary(int32_t kind, int32_t M, const float* mix_cat, const float* mix_an,
                                const float* temperatures, const float* tails, float kappa, const uint32_t* where,
                                int32_t carry, size_t workspace_bytes, const void* const* buffers, int32_t C, int32_t A,
                                int32_t nT, int32_t F, int32_t Mx, impnn_stream_t stream);
int impnn_transfer_mc_grid_summary(const float* u_cat, const float* u_an, const float* image, int64_t image_floats,
                                   const float* multipliers, int32_t S, float kappa, const uint32_t* where, int32_t carry,
                                   size_t workspace_bytes, const void* const* buffers, int32_t C, int32_t A,
                                   impnn_stream_t stream);

/* ---- the Pareto front of two objectives over a cation x anion grid: a sound filter on the GPU, from two planes of
 *      values to a short candidate list that holds the whole front; the caller finishes the front of the candidates.
 *      A pair (i, j) has the float32 values v1, v2 and the keys k1, k2 of the selection's order (the order-preserving
 *      image of the float's bits, -0.0 < +0.0, complemented where largest1 / largest2 is 1: smaller is better) and
 *      flat = i * A + j.  A pair competes if its `where` bit is set (NULL: every pair) and neither value is NaN.  q
 *      dominates p iff k1(q) <= k1(p) and k2(q) <= k2(p) and (k1(q) < k1(p) or k2(q) < k2(p) or flat(q) < flat(p));
 *      the front is the competing pairs no competing pair dominates.
 *      The filter: bucket = (k1 - kmin) >> shift with shift = max(0, bitlength(kmax - kmin) - bits) over the range the
 *      competing pairs span, bits = impnn_pareto_bucket_bits() (14: a 64 KiB table in LDS); table[b] = the smallest k2 of
 *      bucket b; stair[b] = the smallest table entry below b.  A competing pair is dropped iff stair[b] <= k2: a lower
 *      bucket means a strictly smaller k1, so the pair that holds that minimum dominates it.  Every pair of the front
 *      survives; how many others do depends on the data.
 *      Stages.  The planes are given in row-blocks: f1, f2 (rows, A) float32 row-major, where NULL or (rows, W) mask
 *      words (W = impnn_grid_mask_row_words(A)), the rows of one block.  Every stage but begin and staircase is called
 *      once per row-block, in any order of the blocks, and a stage is complete before the next one starts; all calls
 *      go to one stream.  The state is the caller's workspace; the library keeps none.
 *        impnn_pareto_begin      clears the workspace: key range, table, counters
 *        impnn_pareto_range      kmin, kmax of k1 and the number of competing pairs
 *        impnn_pareto_minima     the table; persistent workgroups, each with a private table in LDS, flushed once
 *        impnn_pareto_staircase  stair from table, one workgroup
 *        impnn_pareto_collect    appends the survivors of the block: values (capacity, 2) = (v1, v2) with the inputs'
 *                                bits, cation = row0 + row and anion (capacity) int32.  The count runs on past
 *                                `capacity`; entries beyond it are not written, so a caller that reads a count above
 *                                its capacity repeats the collect stage alone with larger arrays: restart != 0 on the
 *                                first block of such a round sets the count to 0 before the launch.
 *      minima and collect must see the planes, mask and flags range saw (a key outside the range goes to the last
 *      bucket: nothing is written out of bounds, the result is then unspecified).
 *      workspace: impnn_pareto_workspace_bytes bytes, 8-byte aligned.  It opens with impnn_pareto_header, which the
 *      caller may read after a stage: key_min / key_max after range (0xFFFFFFFF / 0 when nothing competes), competing
 *      after range, candidates after collect.
 *      Only integer atomics: range, table, counts and the set of candidates do not depend on the schedule; the order
 *      of the candidate list does.  No float atomics, no workgroup waits for another.
 *      Checks in order (begin and staircase: null pointer, alignment, workspace size): shape (rows, A >= 0, collect: row0,
 *      capacity >= 0) and the largest flags (0 or 1; IMPNN_E_BADARG); zero work (rows == 0 or A == 0: IMPNN_OK, nothing
 *      touched, the count included); null pointers (f1, f2, workspace; the outputs where capacity > 0); alignment
 *      (planes, mask, outputs 4 bytes, workspace 8); the workspace size (IMPNN_E_WORKSPACE); rows * A <= 2^31 - 1 and
 *      row0 + rows <= 2^31 - 1 (IMPNN_E_UNSUPPORTED).  No allocation, no synchronisation. */
typedef struct impnn_pareto_header {
  uint32_t key_min, key_max;
  uint64_t competing, candidates, reserved;
} impnn_pareto_header;
int32_t impnn_pareto_bucket_bits(void);
int impnn_pareto_workspace_bytes(size_t* need);
int impnn_pareto_begin(void* workspace, size_t workspace_bytes, impnn_stream_t stream);
int impnn_pareto_range(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                       void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream);
int impnn_pareto_minima(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                        void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream);
int impnn_pareto_staircase(void* workspace, size_t workspace_bytes, impnn_stream_t stream);
int impnn_pareto_collect(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                         int64_t row0, int32_t restart, float* values, int32_t* cation, int32_t* anion, int64_t capacity,
                         void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream);

/* ---- the applicability domain of a screen: how far a candidate pair lies from anything the model was trained on.
 *      A pair's latent vector is z(i,j) = mix_cat[i] + mix_an[j] (impnn_head_ion_mix rows (C,Mx), (A,Mx); float32, the
 *      cation term first: the bits the head kernels add).  Against a reference set ref (R,Mx) float32, R >= 1:
 *        for p = 0 .. R-1 ascending: d2 = 0; for k ascending: diff = z[k] - ref[p][k]; d2 = fmaf(diff, diff, d2);
 *        the running best starts at (+inf, -1) and is replaced when d2 < best (strict: the lowest p wins among equal d2);
 *        distance = sqrt(best), correctly rounded, nearest = p; if no row ever replaced the initial state (a NaN in the
 *        pair's latent vector): distance NaN, nearest -1.
 *      No |z|^2 - 2 z.r + |r|^2 expansion and no matrix-core product: a pair of the reference set has distance exactly 0.
 *      impnn_domain_grid       distance (C,A) float32 and nearest (C,A) int32 (may be NULL), row-major, int64 indexing:
 *                              C * A may exceed 2^31.
 *      impnn_domain_grid_mask  words (C,W), W = impnn_grid_mask_row_words(A), the pair mask format above: bit (i,j) =
 *                              lo <= distance && distance <= hi as float32 for the distance impnn_domain_grid writes
 *                              (a NaN fails both; an infinity means no limit), pad bits 0, every word written by one
 *                              workgroup.  No C x A float buffer exists.
 *      impnn_domain_rows       the queries are given as rows z (Q,Mx) instead of as a sum -> distance (Q), nearest (Q)
 *                              (may be NULL).  exclude_self != 0: query p skips row p of the reference (needs Q == R):
 *                              every reference row's distance to its nearest other row.
 *      One definition of the inner loop serves the three: an element has the same bits whichever entry produced it.
 *      The reference streams through LDS in chunks of impnn_domain_reference_chunk() rows; the work is 2 * R * Mx lane
 *      operations per pair, the memory traffic C + A + R rows and the output.  1 <= Mx <= 64.
 *      Checks in order: shape (sizes >= 0, Mx >= 1, R >= 1, exclude_self with Q != R, a NaN bound; IMPNN_E_BADARG); Mx <=
 *      64 (IMPNN_E_UNSUPPORTED); zero work (C == 0, A == 0 or Q == 0: IMPNN_OK, nothing touched); null pointers; the
 *      tiles of 16 x 64 pairs must fit one launch (IMPNN_E_UNSUPPORTED).  No allocation, no synchronisation, no state. */
int32_t impnn_domain_reference_chunk(void);
int impnn_domain_grid(const float* mix_cat, const float* mix_an, const float* ref, float* distance, int32_t* nearest,
                      int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream);
int impnn_domain_grid_mask(const float* mix_cat, const float* mix_an, const float* ref, float lo, float hi,
                           uint32_t* words, int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream);
int impnn_domain_rows(const float* z, const float* ref, int32_t exclude_self, float* distance, int32_t* nearest,
                      int32_t Q, int32_t R, int32_t Mx, impnn_stream_t stream);

/* ---- a diverse batch: k pairs of the grid that lie far from the reference set and from each other, by farthest-point
 *      (k-center greedy) selection in the latent space of the domain entries above.
 *      Distance.  z(i,j) = mix_cat[i] + mix_an[j] in float32, the cation term first.  dist(z, r) is the float32 distance
 *      of the domain entries: d2 = 0; for k ascending: diff = z[k] - r[k]; d2 = fmaf(diff, diff, d2); then the correctly
 *      rounded sqrt.  No dot-product expansion, no matrix-core product.
 *      State.  D_0(i,j) is the value impnn_domain_grid writes for ref (R >= 1 rows).
 *      Step, for t = 0 .. k-1:
 *        the candidates are the pairs whose `where` bit is set (where == NULL: all pairs; the pair mask format above,
 *        (C,W) words) and whose D_t > 0: a NaN distance is no candidate, and a pair at distance exactly 0 coincides with
 *        a known or chosen pair and is no candidate either;
 *        the pick p_t is the candidate with the largest float32 D_t, the lowest pair index i * A + j among equal D_t;
 *        D_{t+1} = min(D_t, dist(z, z(p_t))): the value impnn_domain_grid would write against ref plus the rows z(p_0)
 *        .. z(p_t).  The chosen pair's own new distance is exactly 0, so it cannot be picked twice;
 *        with no candidate left the selection ends with n = t < k picks.
 *      Result.  cation[k], anion[k] int32 and distance[k] float32 - each pick's D_t when it was chosen, non-increasing -
 *      with -1 / -1 / NaN in the slots from n on; counts[2] int64: counts[0] = n, counts[1] = the number of candidates
 *      at t = 0.
 *      The order is defined on float32 values because near-ties are the rule on a product grid (z(i,j) - z(i,j') and
 *      z(i',j) - z(i',j') differ by rounding only); the picks do not depend on the schedule: a pick is the maximum of
 *      a 64-bit key (distance bits high, complemented pair index low) by integer atomics.
 *      workspace: impnn_diverse_workspace_bytes(C, A, k) bytes, 16-byte aligned - the (C,A) float32 state, one flag per
 *      tile of 16 x 64 pairs and 4 KiB of records per pick; its content after the call is unspecified.  One launch writes the
 *      state, k - 1 launches of 8 bytes of state traffic per pair follow, each reads its predecessor's pick from the
 *      records; the host does not wait in between.
 *      Limits: 1 <= Mx <= 64, 1 <= k <= impnn_diverse_max_k() (4096: a launch per pick), C * A < 2^32.
 *      Checks in order: shape (sizes >= 0, Mx >= 1, R >= 1) and k < 1 (IMPNN_E_BADARG); Mx <= 64, k and C * A within the
 *      limits (IMPNN_E_UNSUPPORTED); zero work (C == 0 or A == 0: IMPNN_OK, nothing touched); null pointers (where may
 *      be NULL); alignment (workspace 16, counts 8, where 4 bytes); the workspace size (IMPNN_E_WORKSPACE).  No
 *      allocation, no synchronisation, no state. */
int32_t impnn_diverse_max_k(void);
int impnn_diverse_workspace_bytes(int32_t C, int32_t A, int32_t k, size_t* need);
int impnn_diverse_select(const float* mix_cat, const float* mix_an, const float* ref, const uint32_t* where, int32_t k,
                         int32_t* cation, int32_t* anion, float* distance, int64_t* counts, void* workspace,
                         size_t workspace_bytes, int32_t C, int32_t A, int32_t R, int32_t Mx, impnn_stream_t stream);

/*  Mini-batch gather from a device-resident, already padded data set (model.fit over the arrays of
 *  train_viscosity.py:288-314): row rows[r] of tensor t -> row r of dst[t], for up to 8 tensors in one launch.
 *  src / dst / row_bytes are HOST arrays (device pointers, bytes per row: positive multiples of 4); `rows` is a device
 *  int64 array of n_rows indices, not range-checked (the caller built them from a permutation of the data set).
 *  As the first node of a captured training step the host only refreshes `rows` between replays. */
int impnn_gather_rows(int32_t n_tensors, const void* const* src, void* const* dst, const int64_t* row_bytes,
                      const int64_t* rows, int32_t n_rows, impnn_stream_t stream);

/*  Cached frozen steps (data.FrozenStates): the atom states of every distinct ion after its last frozen step live in
 *  one table per ion; a training pass starts from the batch's rows of them.
 *  out[t][b, :] = table[t][rows[t][b], :] for t < n_ions (1 or 2), one launch.  tables / rows / out / row_floats /
 *  table_rows are HOST arrays; rows[t] is a device int32 array of B indices.  row_floats[t] > 0 and a multiple of 4
 *  (16-byte lanes; tables[t] and out[t] 16-byte aligned, rows[t] 4-byte aligned); the two ions may differ in it.  An
 *  index outside [0, table_rows[t]) writes a row of zeros and reads nothing.  B == 0: no launch.  A row is cut into
 *  pieces of 4 KB, one workgroup each; row offsets are 64-bit.  Status: IMPNN_E_BADARG for n_ions outside 1..2, B < 0,
 *  a null pointer, a non-positive or non-multiple-of-4 row_floats, a negative table_rows, a misaligned pointer;
 *  IMPNN_E_UNSUPPORTED where B x pieces exceeds one launch.  There is no backward: the rows are constants of a pass. */
int impnn_state_rows(int32_t n_ions, const float* const* tables, const int32_t* const* rows, float* const* out,
                     const int64_t* row_floats, const int64_t* table_rows, int32_t B, impnn_stream_t stream);

/* ---- f4: backward of the layer-at-a-time path and the optimizer step - what Keras autodiff and
 *      keras.optimizers.Adam(1e-3, clipnorm=1.0) do inside model.fit (train_viscosity.py:227-230,328-338;
 *      train_melting_point.py:205-208).  Every kernel is the adjoint of the forward entry of the same name,
 *      with the same masks and the same "out-of-range index == padding" rule.  Buffers marked (+=) must be
 *      zeroed (or hold a running sum) before the call: they are accumulated with float atomics.
 *
 *  Embedding (a1/a2):        dtable[ids[r],:] (+=) dout[r,:]
 *  Reduce (a5, :57-83):      dmessages[b,e,:] = tgt > 0 ? dagg[b,tgt,:] : 0
 *  GlobalSumPool (a8):       dh[b,n,:] = atom_ids[b,n] > 0 ? dpooled[b,:] : 0
 *  BondMatrixMessage (a4) in the per-bond-type schedule (impnn_bond_type_matrices + impnn_bmm_message_typed):
 *      dh[b,src,:] (+=) A[type]^T dmessages[b,e,:];   dtype_mats[type] (+=) dmessages[b,e,:] (x) h[b,src,:]
 *      (the batch's valid edges are counting-sorted by type in `workspace`, one workgroup per <=64 edges of a type;
 *      sorted_ready != 0: `workspace` still holds the sort of the same (conn, bond_ids) from an earlier call)
 *      then   dW[k] = sum_v Tb[v,k] dtype_mats[v];     dbond_table[v,k] = <dtype_mats[v], W[k]>
 *  GatedUpdate (a7, :142-156): dh, dagg (rows,D) and dparams in the canonical order
 *      Wz 2D*D | bz D | Wr | br | Wh | bh | gamma | beta  (impnn_gated_update_param_floats(D) floats, overwritten);
 *      intermediates are recomputed from (h, agg); the kernel gradients are split-K GEMMs over row chunks and
 *      all parameter sums go through partials in `workspace` (impnn_gated_update_bwd_workspace_floats) that
 *      are added in a fixed order: bitwise reproducible.  atom_dim must divide 256.
 *  `accumulate` != 0 (GatedUpdate dparams; dW and dbond_table of impnn_bond_type_matrices_bwd with K < 64): the
 *      results are ADDED to the output buffers - the caller points them at the optimizer's gradient buffer and
 *      saves one add per parameter tensor. */
int impnn_embed_gather_bwd(const int32_t* ids, const float* dout, float* dtable, int64_t rows, int32_t vocab,
                           int32_t dim, impnn_stream_t stream);
int impnn_reduce_scatter_bwd(const float* dagg, const int32_t* tgt, int32_t tgt_stride, float* dmessages, int32_t B,
                             int32_t N, int32_t E, int32_t D, impnn_stream_t stream);
int impnn_global_sum_pool_bwd(const float* dpooled, const int32_t* atom_ids, float* dh, int32_t B, int32_t N,
                              int32_t D, impnn_stream_t stream);
/*  The gradient of the LISTED rows of an embedding table, and of no other row (a frozen Embedding with trainable_rows;
 *  csrc/embed_rows.hip).  For each listed token v = row_list[i], i < n_listed:
 *      dtable[v,:] = (accumulate ? dtable[v,:] : +0.0) + sum over the r < rows with ids[r] == v of dout[r,:]
 *  Rows of dtable that the list does not name are NOT written (nor read).  ids == NULL is the identity, rows == vocab
 *  and row r holds token r: the listed rows of a full (vocab, dim) gradient are moved (or added) into dtable.
 *  Indices are not trusted: a listed id outside [0, vocab) is skipped, an id the list holds twice counts once, an ids[r]
 *  outside [0, vocab) is padding.
 *  The sum has one order, a function of `rows` alone: the rows in chunks of 64, chunk c to wave c mod 8 of the token's
 *  workgroup, a wave's rows in ascending order from +0.0, then the eight waves' partials in wave order, then the old
 *  value.  No float atomics: the same call gives the same bits on every run (impnn_embed_gather_bwd does not).
 *  buffers: a HOST table of one device pointer, [0] = dtable (vocab, dim) float32.  Any dim >= 1, any rows >= 0; ids,
 *  dout, row_list and dtable 4-byte aligned.
 *  Checks in order: shape (rows, n_listed, dim >= 0, vocab > 0, accumulate 0 or 1, ids == NULL only with rows == vocab;
 *  IMPNN_E_BADARG); zero work (n_listed == 0, rows == 0 or dim == 0: IMPNN_OK, nothing touched); null pointers (the
 *  table and its entry, dout, row_list); 4-byte alignment; n_listed * ceil(dim / 64) < 2^31 (IMPNN_E_UNSUPPORTED).  No
 *  allocation, no synchronisation, no state. */
int impnn_embed_rows_bwd(const int32_t* ids, const float* dout, const int32_t* row_list, int32_t n_listed,
                         const void* const* buffers, int64_t rows, int32_t vocab, int32_t dim, int32_t accumulate,
                         impnn_stream_t stream);
int64_t impnn_bmm_message_typed_bwd_workspace_bytes(int32_t B, int32_t E, int32_t Vb);
/*  impnn_bmm_message_typed (forward) over the same type-sorted edge segments, any D <= 128: A[type] staged in LDS,
 *  one workgroup per <= 64 edges of a type.  Same workspace (and size query) as the backward entry: a sort made here
 *  serves the backward call of the layer and every other layer of the ion (sorted_ready = 1 there).
 *  sorted_ready | 2: `messages` is the buffer an earlier call on the SAME (bond_ids, conn) wrote and nothing else
 *  touched since - the zero rows of masked / out-of-range edges (models/layers.py:114-115) are still in place and
 *  the pass that writes them is skipped (a training loop that keeps one message buffer per ion for all its layers). */
int impnn_bmm_message_typed_sorted(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                   const float* type_mats, float* messages, void* workspace, int64_t workspace_bytes,
                                   int32_t B, int32_t N, int32_t E, int32_t D, int32_t Vb, int32_t sorted_ready,
                                   impnn_stream_t stream);
int impnn_bmm_message_typed_bwd(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                const float* type_mats, const float* dmessages, float* dh, float* dtype_mats,
                                void* workspace, int64_t workspace_bytes, int32_t B, int32_t N, int32_t E, int32_t D,
                                int32_t Vb, int32_t sorted_ready, impnn_stream_t stream);
/*  Backward of Reduce o BondMatrixMessage in one launch (models/layers.py:57-83 after :100-117): the gradient of a
 *  message IS the gradient of the aggregate row it was added to, so the (B,E,D) message gradient is never
 *  materialised - the kernel reads dagg (B,N,D) at row tgt(e).  Otherwise identical to impnn_bmm_message_typed_bwd. */
int impnn_message_reduce_typed_bwd(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                   const float* type_mats, const float* dagg, float* dh, float* dtype_mats,
                                   void* workspace, int64_t workspace_bytes, int32_t B, int32_t N, int32_t E,
                                   int32_t D, int32_t Vb, int32_t sorted_ready, impnn_stream_t stream);
/*  The same with a (B,E,D) buffer whose rows at masked / out-of-range edges are ZERO - the message buffer an
 *  impnn_bmm_message_typed_sorted call of the same (bond_ids, conn) left behind is one (its other rows are overwritten
 *  here).  The per-edge vectors A_t^T g_e go to their edge slot's row and a slot-order pass adds them into dh at the
 *  source rows - no float atomics on dh (22 M of them at atom_dim 128, batch 4096: 260 of the kernel's 349 us), and
 *  dh becomes bitwise reproducible. */
int impnn_message_reduce_typed_bwd_scratch(const float* h, const int32_t* bond_ids, const int32_t* conn,
                                           const float* type_mats, const float* dagg, float* dh, float* dtype_mats,
                                           void* workspace, int64_t workspace_bytes, float* edge_scratch, int32_t B,
                                           int32_t N, int32_t E, int32_t D, int32_t Vb, int32_t sorted_ready,
                                           impnn_stream_t stream);
int impnn_bond_type_matrices_bwd(const float* bond_table, const float* W, const float* dtype_mats, float* dW,
                                 float* dbond_table, int32_t Vb, int32_t K, int32_t D, int32_t accumulate,
                                 impnn_stream_t stream);
/*  The per-bond-type matrices of ALL message layers of a model (both ions, every step) in one launch, and their
 *  backward in two: `W`, `type_mats`, `dtype_mats`, `dW` are host arrays of n device pointers (layer p: W_p (K,D,D),
 *  A_p (Vb,D,D)); the bond embedding table is shared (train_viscosity.py:172), so dbond_table (Vb,K) is the sum over
 *  the layers, accumulated in layer order.  accumulate as in impnn_bond_type_matrices_bwd.  Same arithmetic per layer
 *  as the single-layer entries (bitwise equal A_p and dW_p).  A training step at the reference's batch 32 is bound by
 *  the number of launches: 3 launches here replace 3 per layer. */
int impnn_bond_type_matrices_multi(const float* bond_table, const float* const* W, float* const* type_mats,
                                   int32_t n, int32_t Vb, int32_t K, int32_t D, impnn_stream_t stream);
int impnn_bond_type_matrices_multi_bwd(const float* bond_table, const float* const* W,
                                       const float* const* dtype_mats, float* const* dW, float* dbond_table,
                                       int32_t n, int32_t Vb, int32_t K, int32_t D, int32_t accumulate,
                                       impnn_stream_t stream);
/* The same with a workspace (impnn_bond_type_matrices_multi_bwd_workspace_floats floats, 16-byte aligned): the bond-table
 * gradient - a (Vb x K) result over a contraction of n D^2 - runs on the matrix cores, per-wave partials in the
 * workspace, added in a fixed order (bitwise reproducible; 116-170 us -> ~15 us at atom_dim 128, all of it on the
 * critical path of a training step).  K <= 16, Vb <= 128, D % 16 == 0; other shapes take the entry above's kernels. */
int64_t impnn_bond_type_matrices_multi_bwd_workspace_floats(int32_t n, int32_t Vb, int32_t K, int32_t D);
int impnn_bond_type_matrices_multi_bwd_ws(const float* bond_table, const float* const* W,
                                          const float* const* dtype_mats, float* const* dW, float* dbond_table,
                                          int32_t n, int32_t Vb, int32_t K, int32_t D, int32_t accumulate,
                                          float* workspace, int64_t workspace_floats, impnn_stream_t stream);
/* One launch: *snapshot = *counter; *counter += 1 (both DEVICE int64).  A training pass takes its step this way, so
 * the step never passes through the host and a captured pass advances it on every replay. */
int impnn_dropout_step(int64_t* counter, int64_t* snapshot, impnn_stream_t stream);
/* The mask itself (tests, diagnostics): out[row * D + c] = scale or 0 for the rows row_index[0 .. *n_rows) (both NULL:
 * rows 0 .. max_rows), as the entries above draw it; other rows of out are not written. */
int impnn_dropout_mask(uint64_t seed, const int64_t* step, int32_t layer_word, float rate, const int32_t* row_index,
                       const int32_t* n_rows, int64_t max_rows, int32_t D, float* out, impnn_stream_t stream);

/*  Optimizer step, one launch for all variables (train_viscosity.py:227-230):
 *      g <- g * clipnorm / max(||g||_2, clipnorm)      per variable (tf.clip_by_norm); clipnorm <= 0: off
 *      m <- b1 m + (1-b1) g;   v <- b2 v + (1-b2) g^2
 *      w <- w - lr * sqrt(1 - b2^step) / (1 - b1^step) * m / (sqrt(v) + eps)         (step counts from 1)
 *  var_table: DEVICE array of 4*n_vars device pointers (w, g, m, v per variable, all f32);
 *  sizes: DEVICE array of n_vars element counts. */
int impnn_adam_clipnorm_step(const void* var_table, const int64_t* sizes, int32_t n_vars, int64_t step, float lr,
                             float beta1, float beta2, float eps, float clipnorm, impnn_stream_t stream);
/*  The same with the step number in DEVICE memory: *step_counter is incremented by one (on the stream) and the
 *  new value is the `step` of this update.  A training step captured in a hipGraph (forward, backward and this
 *  call) then advances its own counter on every replay. */
int impnn_adam_clipnorm_step_counted(const void* var_table, const int64_t* sizes, int32_t n_vars,
                                     int64_t* step_counter, float lr, float beta1, float beta2, float eps,
                                     float clipnorm, impnn_stream_t stream);
/*  The same with the learning rate in DEVICE memory too, plus tf.clip_by_global_norm and keras's decoupled weight
 *  decay.  lr_record: a caller-owned device record of 32 four-byte words (i32 or f32 as marked), 4-byte aligned:
 *      word 0   i32  kind: 0 constant, 1 ExponentialDecay, 2 CosineDecay, 3 PiecewiseConstantDecay
 *      word 1   i32  flags: bit 0 = staircase (ExponentialDecay)
 *      word 2   f32  lr (constant) / initial_learning_rate
 *      word 3   f32  decay_rate (ExponentialDecay) / alpha (CosineDecay)
 *      word 4   i32  decay_steps (> 0)
 *      word 5   i32  warmup_steps (CosineDecay; 0: no warm-up)
 *      word 6   f32  CosineDecay: the rate the cosine starts from (warmup_target, or word 2 again without one)
 *      word 7   i32  PiecewiseConstantDecay: number of boundaries, 0 .. 8
 *      8..15    i32  boundaries, increasing
 *      16..24   f32  values: values[i] while s <= boundaries[i], values[count] after the last boundary
 *      25..31        reserved, 0
 *  The kernel forms the rate of the update itself: with s = *step_counter - 1 after the increment (the updates
 *  already applied; keras reads its schedule at `iterations` before the update, the bias correction uses s + 1),
 *      constant     lr
 *      exponential  lr0 * decay_rate ^ (s / decay_steps), floor(s / decay_steps) with staircase
 *      cosine       s < warmup_steps: lr0 + (target - lr0) * s / warmup_steps;  else with s' = s - warmup_steps
 *                   target * ((1 - alpha) * 0.5 * (1 + cos(pi * min(s', decay_steps) / decay_steps)) + alpha)
 *      piecewise    as above
 *  in f32.  The host changes the rate by writing the record on the stream (no argument is frozen into a captured
 *  graph).  The record is not validated by this entry (it is device memory): impnn_lr_schedule_check validates a
 *  HOST copy before upload; a kind the kernel does not know gives a NaN rate.
 *  clipnorm: per variable as above; global_clipnorm > 0: g <- g * c / max(||g||_global, c) over all variables of the
 *  call (both > 0: IMPNN_E_BADARG).  A launch ahead of the update writes the sum of squares of every (variable,
 *  slice) into `workspace` (impnn_adam_step_scheduled_workspace_floats(n_vars) floats, needed only with
 *  global_clipnorm); every workgroup of the update adds them in index order - no float atomics, one scale for all
 *  elements, the same bits on every run.  An all-zero gradient gives scale 1; a non-finite global norm makes every
 *  update of that step NaN (w, m, v), as tf.clip_by_global_norm does.
 *  weight_decay > 0: w <- w - lr_s * weight_decay * w ahead of the Adam update, with the step's rate lr_s, for the
 *  variables whose word in decay_flags (DEVICE, n_vars i32) is non-zero. */
int64_t impnn_adam_step_scheduled_workspace_floats(int32_t n_vars);
int impnn_adam_step_scheduled(const void* var_table, const int64_t* sizes, int32_t n_vars, int64_t* step_counter,
                              const void* lr_record, float beta1, float beta2, float eps, float clipnorm,
                              float global_clipnorm, float weight_decay, const int32_t* decay_flags, float* workspace,
                              int64_t workspace_floats, impnn_stream_t stream);
/*  Validates a HOST copy of a learning-rate record (32 words): IMPNN_E_UNSUPPORTED for an unknown kind or more than
 *  8 boundaries, IMPNN_E_BADARG for decay_steps <= 0, a negative decay_rate, boundaries out of order or a
 *  non-finite value. */
int impnn_lr_schedule_check(const void* host_record);
/*  out[i] = the rate the update kernel would use at s = steps[i] (DEVICE pointers; the kernel's own function). */
int impnn_lr_schedule_eval(const void* lr_record, const int64_t* steps, float* out, int32_t n, impnn_stream_t stream);

/* ---- regression metrics: segmented sums of (pred, y, sample_weight) in fp64 (csrc/metrics.hip), from which the host
 *      forms MAE, MSE, RMSE, bias, the maximal error and R^2 (ionic_mpnn_amd.train, compile(metrics=...)).
 *  The n samples are cut into n_seg segments: segment s holds the samples b = order[k] for
 *  seg_offsets[s] <= k < seg_offsets[s + 1] (seg_offsets: DEVICE, n_seg + 1 ascending values in [0, n]; NULL with
 *  n_seg == 1 is the one segment [0, n); order: DEVICE, n indices in [0, n), NULL is the identity).  Per sample, every
 *  operation in fp64 on the converted float32 values,
 *      e = scale * (pred[b] - y[b]),  yr = offset + scale * y[b],  w = sample_weight[b]  (NULL: w = 1)
 *  (offset and scale carry a standardised target back to its unit), and a segment's record of
 *  impnn_regression_sums_words() = 8 doubles is
 *      0  the number of samples         4  sum w * (e * e)
 *      1  sum w                         5  sum w * yr
 *      2  sum w * e                     6  sum w * (yr * yr)
 *      3  sum w * |e|                   7  max |e| over the samples with w > 0: NaN if one of those e is NaN, 0 for an
 *                                          empty segment
 *  sums: DEVICE, n_seg x 8 doubles.  accumulate == 0 overwrites them; accumulate != 0 adds words 0..6 to what they hold
 *  and word 7 takes the maximum (a NaN stays): one thread per word does the read-modify-write, calls are ordered by
 *  the stream, no atomic.  An empty segment writes, or adds, zeros.
 *  Order of the additions: a thread adds its elements in index order, then lanes, waves by a fixed tree; a segment
 *  belongs to one wave (n / n_seg <= 512) or one workgroup, a single segment to one wave (n <= 64) or one workgroup
 *  of 256 (n <= 16384) or 1024 threads - correct at any n, fast where a training step or a table of short segments
 *  needs it.  The path follows (n, n_seg) alone, never the data: the same call gives the same bits.  No product is
 *  contracted into an addition, so every term is the double the host reference forms.  No workspace, no allocation,
 *  no synchronisation.  A position or an index outside [0, n) is not read (the result is then unspecified).
 *  Status codes, in this order: IMPNN_E_BADARG for n < 0, n_seg < 1, a null pred / y / sums, a null seg_offsets with
 *  n_seg > 1, a misaligned pointer (4 bytes: pred, y, sample_weight, order; 8 bytes: seg_offsets, sums), a scale that
 *  is zero or not finite, an offset that is not finite, order with n >= 2^31; then n == 0 with one segment is
 *  IMPNN_OK (nothing is launched under accumulate, the record is zeroed otherwise).  No IMPNN_E_UNSUPPORTED case. */
int64_t impnn_regression_sums_words(void);
int impnn_regression_sums(const float* pred, const float* y, const float* sample_weight, const int32_t* order,
                          const int64_t* seg_offsets, int64_t n, int32_t n_seg, double offset, double scale,
                          int32_t accumulate, double* sums, impnn_stream_t stream);

/* ---- measurement: HIP-event timing of the dominant kernel (encoder_fused_kernel / encoder_typed_kernel), recorded on the
 *      stream the kernel is launched on.  After impnn_profile_enable(capacity) every
 *      impnn_encoder_fused call of this thread records one (start, stop) event pair around that
 *      kernel alone (the two small plan kernels are outside the pair) until `capacity` pairs exist.
 *      impnn_profile_collect synchronises the recorded events, writes up to max_n durations in
 *      milliseconds, returns their count in *n_out and rewinds.  Used by bench.py's roofline leg. */
int impnn_profile_enable(int32_t capacity);
int impnn_profile_collect(float* ms_out, int32_t max_n, int32_t* n_out);
int impnn_profile_disable(void);

/* ---- diagnostics: when a device buffer of >= 256 bytes per encoder workgroup is set, the encoder
 *      kernel's lane 0 writes s_memtime stamps into it (entry, after prologue, after each of the
 *      first 5 steps, exit, and the phase boundaries of wave 0's first tile in one step) -
 *      32 uint64 per workgroup.  NULL (the default) disables it; with NULL
 *      no stamp instruction executes.  Never set during a timed run. */
int impnn_debug_set_stamp_buffer(void* device_buffer, size_t bytes);

/* ---- debug: counts indices the reference's CPU path would raise on.  counts[0] += #conn
 *      entries outside [0,N), counts[1] += #atom ids outside [0,Va), counts[2] += #bond ids
 *      outside [0,Vb).  Any of conn/atom_ids/bond_ids may be NULL.  counts: 3 device int32,
 *      zeroed by the caller. */
int impnn_validate_indices(const int32_t* conn, const int32_t* atom_ids, const int32_t* bond_ids,
                           int32_t* counts, int32_t B, int32_t N, int32_t E, int32_t Va,
                           int32_t Vb, impnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IMPNN_H_ */
