// Fused message-passing encoder, per-bond-type form (mode 2 "f32t"), gfx950 / MI355X: encode() of
// train_viscosity.py:166-187 and train_melting_point.py:152-171 up to and including GlobalSumPool, both ions in
// one launch, atom_dim 32, ANY bond_dim (K = 8 of the viscosity model, K = D^2 = 1024 of the melting-point model).
//
// Same frame as encoder_fused.hip - persistent 1024-thread workgroups, chunks of <= 256 packed atom rows whose
// graph structure arrives as a record built by the plan kernels, node state h in LDS for all S steps, GatedUpdate
// as transposed f32-MFMA GEMMs with atoms on the MFMA N dimension - but the message is computed the way the
// reference orders it (models/layers.py:108-112): A_e = sum_k bond_state[e,k] W[k], then m_e = A_e h[src_e].
// bond_state is always an Embedding lookup (train_viscosity.py:172), so A_e is one of Vb matrices
// A[v] = sum_k bond_table[v,k] W[k], prepared once per weight version (encoder_plan.hip: typed_image).
//
//   message phase (all 16 waves): the chunk's valid edges are grouped by bond type in groups of <= 4; a group is
//     16 x v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 blocks: 8 feature quads x 2 halves of k), exact f32
//     products, the edge operand broadcast inside the instruction (CBSZ/ABID), the matrix operand straight from L2
//     once per type and chunk-step.  Messages are written to an LDS buffer in jagged-diagonal order.
//   atom phase (one 16-atom tile per wave): agg[a] = sum of the row's in-edge messages in edge-slot order (the
//     reference's sequential scatter_nd, models/layers.py:78-82; slot(row, d) = jdptr[d] + row, so a tile's reads
//     of one d are 16 consecutive slots: conflict-free), then GatedUpdate (models/layers.py:142-156) exactly as in
//     encoder_fused.hip's f32 mode, h updated in place.
//
//   step 0: h[src] is atom_table[atom id] (or zeros), so its messages depend on the weights alone; an image prepared with
//     the atom table carries them as a table (encoder_layout.h: M0Header), and its rows travel L2 -> LDS by
//     global_load_lds, addressed by the plan's slot-ordered source list, while the PREVIOUS chunk is pooled; step 0's
//     update image goes the same way.  The same holds for the z / r gate accumulators after their h half (bias + W_h h):
//     an image of the with-gates entry carries them as a second table (G0Header) and step 0's atom phase loads a row.
//     With both tables nothing fills the h buffer for step 0: a tile's wave takes its rows' h quads into registers in front
//     of the prologue barrier and runs that step's atom phase outside the step loop, without a mid-step barrier.
//
// MFMA work per row is 12 D^2 (update) + 2 D^2 per in-edge, against (12 + 2 K) D^2 per row in the pull form:
// 2.7 kflop instead of 28.7 kflop per row for the message at bond_dim 8 and 1.7 in-edges per row.
#include <type_traits>

#include "encoder_device.h"
#include "encoder_layout.h"
#include "kernel_device.h"

namespace impnn {
namespace enc {

namespace {

constexpr int kOffUpd = 0;
constexpr int off_h(bool x3) { return kOffUpd + (x3 ? kXUpdLds : kTUpdLds); }
// hs: the LDS row stride of h - kTHS (36: rows spread over the banks), or 32 where mode 3 meets 640-edge chunks (explicit-
// hydrogen shapes, E > 512): the three-plane update image and 642 message slots leave no room for the padding
constexpr int kTHSBig3 = 32;
constexpr int off_msg(bool x3, int hs = kTHS) { return off_h(x3) + kRCap * hs; }
constexpr int off_rec(bool x3, int ecap, int hs = kTHS) { return off_msg(x3, hs) + tmsg_floats(ecap); }
// then: the record (trec_lds_bytes(Vb, ecap)) and, when it fits, the atom table ((Va + 1) rows of kTAS floats)
constexpr size_t lds_fixed_bytes(bool x3, int Vb, int ecap, int hs = kTHS) {
  return sizeof(float) * (size_t)off_rec(x3, ecap, hs) + trec_lds_bytes(Vb, ecap);
}
static_assert(lds_fixed_bytes(true, kTVbMax, kTECap) <= 160 * 1024 && lds_fixed_bytes(false, kTVbMax, kTECapBig) <= 160 * 1024 &&
                  lds_fixed_bytes(true, kTVbMax, kTECapBig, kTHSBig3) <= 160 * 1024,
              "LDS budget");

// ---- mode 3 ("f32x3"): f32 GEMM products on the bf16 matrix pipe without narrowing them.  An f32 value is the exact
// sum of three bf16 terms (bf16 keeps fp32's exponent; 3 x 8 significant bits): b0 = the upper half of the word, b1 =
// the upper half of the exact residual x - b0, b2 = what is left (<= 8 bits).  All nine cross products of two such
// triples are exact in the MFMA's f32 accumulator, so a GEMM differs from the f32-MFMA one only in the order the
// (exact) products are added.  v_mfma_f32_16x16x32_bf16 is 16 cycles for 32 k; nine of them replace eight
// v_mfma_f32_16x16x4_f32 of 32 cycles - on a pipe that, unlike the f32 one, co-executes with the VALU.
typedef bf16x8_t bf16x8;  // (kernel_device.h)
struct B3 {
  bf16x8 p0, p1, p2;
};
// Non-finite operands: a NaN stays a NaN through its first term.  An INFINITY splits into (inf, inf - inf = nan, nan), so
// every product it meets is NaN, where exact f32 arithmetic has w * inf = +-inf and a saturating gate may even turn that
// back into a finite number (sigmoid(+inf) = 1).  This cannot be repaired inside the split - with (inf, 0, 0) the terms
// a1 * inf of weights whose residual a1 is exactly 0 are NaN again - so mode 3 is the more conservative of the two: the
// rows it reports non-finite are a superset of mode 2's, and a finite row equals mode 2's up to summation order
// (tests/test_gpu_encoder.py::test_f32x3_propagates_nan_and_inf_like_f32t; measured: guarding the split costs 4 us per
// 4096-pair launch and still leaves the 0 * inf terms).
// (split_pair, kernel_device.h: two values -> their three packed bf16 pairs)
__device__ __forceinline__ B3 split8x3(f32x4 a, f32x4 b) {
  union {
    bf16x8 v;
    unsigned u[4];
  } q0, q1, q2;
  split_pair(a[0], a[1], q0.u[0], q1.u[0], q2.u[0]);
  split_pair(a[2], a[3], q0.u[1], q1.u[1], q2.u[1]);
  split_pair(b[0], b[1], q0.u[2], q1.u[2], q2.u[2]);
  split_pair(b[2], b[3], q0.u[3], q1.u[3], q2.u[3]);
  B3 r;
  r.p0 = q0.v;
  r.p1 = q1.v;
  r.p2 = q2.v;
  return r;
}
// c0 += W0 b, c1 += W1 b (W: three planes at blk, blk + 512, blk + 1024): all nine cross products, smallest first, the
// two accumulator chains interleaved (a dependent v_mfma_f32_16x16x32_bf16 waits ~4 cycles for its predecessor).
__device__ __forceinline__ void mma9x2(f32x4& c0, f32x4& c1, const __bf16* blk0, const __bf16* blk1, int lane, const B3& b) {
  const bf16x8 a00 = *reinterpret_cast<const bf16x8*>(blk0 + lane * 8);
  const bf16x8 a01 = *reinterpret_cast<const bf16x8*>(blk0 + 512 + lane * 8);
  const bf16x8 a02 = *reinterpret_cast<const bf16x8*>(blk0 + 1024 + lane * 8);
  const bf16x8 a10 = *reinterpret_cast<const bf16x8*>(blk1 + lane * 8);
  const bf16x8 a11 = *reinterpret_cast<const bf16x8*>(blk1 + 512 + lane * 8);
  const bf16x8 a12 = *reinterpret_cast<const bf16x8*>(blk1 + 1024 + lane * 8);
  c0 = mfma_bf16(a02, b.p2, c0);  c1 = mfma_bf16(a12, b.p2, c1);
  c0 = mfma_bf16(a01, b.p2, c0);  c1 = mfma_bf16(a11, b.p2, c1);
  c0 = mfma_bf16(a02, b.p1, c0);  c1 = mfma_bf16(a12, b.p1, c1);
  c0 = mfma_bf16(a00, b.p2, c0);  c1 = mfma_bf16(a10, b.p2, c1);
  c0 = mfma_bf16(a02, b.p0, c0);  c1 = mfma_bf16(a12, b.p0, c1);
  c0 = mfma_bf16(a01, b.p1, c0);  c1 = mfma_bf16(a11, b.p1, c1);
  c0 = mfma_bf16(a00, b.p1, c0);  c1 = mfma_bf16(a10, b.p1, c1);
  c0 = mfma_bf16(a01, b.p0, c0);  c1 = mfma_bf16(a11, b.p0, c1);
  c0 = mfma_bf16(a00, b.p0, c0);  c1 = mfma_bf16(a10, b.p0, c1);
}

// v_mfma_f32_4x4x1_16b_f32 with CBSZ = 3: the 16 blocks form two groups of 8 (lanes 0-31 / 32-63) and every block of a
// group takes its A operand from block ABID of the group.  So ONE register carries the A operands of EIGHT
// instructions: the 4 lanes of block b hold what instruction ABID = b multiplies.
template <int ABID>
__device__ __forceinline__ f32x4 mfma1(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 3, ABID, 0);
}

// One group of the message phase: its record entry and the A operands of its 16 MFMAs - lane l = 32 kh + 4 b + i holds
// h[source row of edge i][16 kh + 2 b] and [.. + 2 b + 1]: one ds_read_b64 per lane, no lane idle, two registers.
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
// global_load_lds_dwordx4: lane l's 16 bytes at gsrc -> LDS at dst + 16 l (dst: wave-uniform), no register in between.
// As an asm statement, not as __builtin_amdgcn_global_load_lds: the compiler orders a transfer it knows of against EVERY
// later LDS access it cannot tell apart from the destination - it waited vmcnt(0) between any two transfers into the message
// buffer and in front of the pool's first LDS read, which is the overlap this is for.  A transfer issued here is unknown
// to the compiler's s_waitcnt bookkeeping (its own counted waits only become longer: loads return in order), so whoever
// reads the destination waits vmcnt(0) explicitly, then a barrier, then reads.  M0 is the compiler's: saved and restored;
// the s_nop is the wait state between a scalar write of M0 and a vector-memory instruction that reads it.
__device__ __forceinline__ void glds16(const void* gsrc, const float* dst) {
  const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_ptr_t)dst);
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
struct Grp {
  uint4 ge;
  f32x2v aq;
};
// One type run: the matrix rows of this lane, and the run's first group (requested as soon as the run is known).
struct Run {
  f32x4 bq[4];
  Grp first;
};

// The messages of one group: 16 MFMAs on two accumulator chains, the two k-halves joined by one v_permlane32_swap per
// edge pair.  aq: the lane's two h values (see Grp); bq: the lane's half row of the type matrix.  Returns, for feature
// l & 31, the message of edge l >> 5 (m01) and of edge 2 + (l >> 5) (m23).  Nothing in a 4x4x1 block depends on the other
// edges of the group, so an edge's message is a function of (type matrix, source row) alone - which is what lets the
// step-0 table kernel below reproduce the message phase's bits by calling this very function.
__device__ __forceinline__ void group_messages(const f32x2v aq, const f32x4 (&bq)[4], float& m01, float& m23) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#ifndef IMPNN_DIAG_NO_MSG_MFMA  // (diagnostics builds only: wrong results)
  // instruction k (= h column 16 kh + k): A from register k & 1, block k >> 1; B = the lane's matrix element k.
  // (Two accumulator chains; four were measured: +4 % kernel time, the registers cost more than the s_nops.)
  acc0 = mfma1<0>(aq[0], bq[0][0], acc0);
  acc1 = mfma1<0>(aq[1], bq[0][1], acc1);
  acc0 = mfma1<1>(aq[0], bq[0][2], acc0);
  acc1 = mfma1<1>(aq[1], bq[0][3], acc1);
  acc0 = mfma1<2>(aq[0], bq[1][0], acc0);
  acc1 = mfma1<2>(aq[1], bq[1][1], acc1);
  acc0 = mfma1<3>(aq[0], bq[1][2], acc0);
  acc1 = mfma1<3>(aq[1], bq[1][3], acc1);
  acc0 = mfma1<4>(aq[0], bq[2][0], acc0);
  acc1 = mfma1<4>(aq[1], bq[2][1], acc1);
  acc0 = mfma1<5>(aq[0], bq[2][2], acc0);
  acc1 = mfma1<5>(aq[1], bq[2][3], acc1);
  acc0 = mfma1<6>(aq[0], bq[3][0], acc0);
  acc1 = mfma1<6>(aq[1], bq[3][1], acc1);
  acc0 = mfma1<7>(aq[0], bq[3][2], acc0);
  acc1 = mfma1<7>(aq[1], bq[3][3], acc1);
#else
  acc0[0] = aq[0] + bq[0][0] + bq[3][3];
  acc1[1] = aq[1] + bq[1][1] + bq[2][2];
#endif
  // acc0 + acc1 as four v_add_f32: as a vector add the compiler emits two v_pk_add_f32, which beside MFMAs cost
  // more issue time than the four scalar adds (the same IEEE sums either way)
  float x0 = acc0[0] + acc1[0], x1 = acc0[1] + acc1[1], x2 = acc0[2] + acc1[2], x3 = acc0[3] + acc1[3];
  // element i of lane l: edge i, feature l & 31, k-half l >> 5.
  // v_permlane32_swap x, y: lanes 32-63 of x <-> lanes 0-31 of y.  Afterwards x = {x.lo, y.lo},
  // y = {x.hi, y.hi}, so x + y is edge 0 (2) complete in lanes 0-31 and edge 1 (3) in lanes 32-63.
  // (Inline asm: the compiler's builtin for this gfx950 instruction folded its two operands into one here.
  //  The s_nop covers the VALU-write -> permlane-read wait states the assembler does not insert.)
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3"
               : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
  m01 = x0 + x1;
  m23 = x2 + x3;
}

// Step-0 message table (encoder_layout.h: M0Header): one wave per (bond type v, four consecutive atom ids), fed exactly
// like a group of the message phase - lane l = 32 kh + 4 b + i holds atom_table[a0 + i][16 kh + 2 b] and [.. + 1] (zeros
// for a0 + i >= Va: column Va is the zero row, beyond it padding), the matrix rows come from step 0's type matrices in
// the image - so M0[v][a] carries the bits the message phase writes, 0 * inf = NaN in column Va included.
__global__ __launch_bounds__(256) void typed_m0_kernel(const float* tmat0, const float* atom_table, float* m0,
                                                       M0Header* hdr, int Va, int Vb, int S) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int nga = (Va + 4) >> 2;  // groups of four among the Va + 1 columns
  if (w < Vb * nga) {
    const int v = w / nga, a0 = 4 * (w - v * nga);
    const int kh = lane >> 5, f = lane & 31;
    const int ai = a0 + (lane & 3);
    f32x2v aq = {0.f, 0.f};
    if (ai < Va) aq = *reinterpret_cast<const f32x2v*>(atom_table + (size_t)ai * kD + 16 * kh + 2 * ((lane >> 2) & 7));
    const float* bp = tmat0 + (size_t)v * kTMatFloats + kh * 512 + f * 4;
    f32x4 bq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bq[i] = ld4(bp + i * 128);
    float m01, m23;
    group_messages(aq, bq, m01, m23);
    float* row = m0 + (size_t)v * (Va + 1) * kD + f;
    if (a0 + kh <= Va) row[(size_t)(a0 + kh) * kD] = m01;
    if (a0 + 2 + kh <= Va) row[(size_t)(a0 + 2 + kh) * kD] = m23;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *hdr = M0Header{kM0Magic, Va, Vb, S};
}

// The h half of the gates z and r (models/layers.py:144-147): bias, then W_h h, for the 16 rows of a tile - lane (a, q)
// holds h[row a][4 q ..] (h0) and [16 + 4 q ..] (h1) and receives the accumulators of the same features.  wupd / wvec: an
// update image and its vectors, in LDS (the atom phase) or in global memory (typed_g0_kernel below): one body for both,
// as group_messages is for the messages, so that a row of the step-0 gate table holds the bits the atom phase computes.
// Mode 3: the two mma9x2 on split8x3(h); mode 2: the half == 0 turns of the gate loop.
template <bool X3>
__device__ __forceinline__ void gates_h_half(const float* wupd, const float* wvec, int lane, int q, const f32x4 h0,
                                             const f32x4 h1, f32x4& z0, f32x4& z1, f32x4& r0, f32x4& r1) {
  z0 = ld4(wvec + 0 * kD + 4 * q), z1 = ld4(wvec + 0 * kD + 16 + 4 * q);
  r0 = ld4(wvec + 1 * kD + 4 * q), r1 = ld4(wvec + 1 * kD + 16 + 4 * q);
  if constexpr (X3) {
    // (mode 3's A operands: block ((gate*2 + T)*2 + half) of the image, 3 x 512 bf16)
    const __bf16* const wb = reinterpret_cast<const __bf16*>(wupd);
    const B3 sh = split8x3(h0, h1);
    mma9x2(z0, z1, wb + ((0 * 2 + 0) * 2 + 0) * 1536, wb + ((0 * 2 + 1) * 2 + 0) * 1536, lane, sh);
    mma9x2(r0, r1, wb + ((1 * 2 + 0) * 2 + 0) * 1536, wb + ((1 * 2 + 1) * 2 + 0) * 1536, lane, sh);
  } else {
    // A operands: block ((gate*2 + T)*2 + half)*2 + u of the image, 16 B per lane, lane-linear (conflict-free)
    const float* wl = wupd + 4 * lane;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4 Az0 = ld4(wl + ((0 * 2 + 0) * 4 + u) * 256);
      const f32x4 Az1 = ld4(wl + ((0 * 2 + 1) * 4 + u) * 256);
      const f32x4 Ar0 = ld4(wl + ((1 * 2 + 0) * 4 + u) * 256);
      const f32x4 Ar1 = ld4(wl + ((1 * 2 + 1) * 4 + u) * 256);
      const f32x4 Bv = u == 0 ? h0 : h1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        z0 = mfma4(Az0[r], Bv[r], z0);
        z1 = mfma4(Az1[r], Bv[r], z1);
        r0 = mfma4(Ar0[r], Bv[r], r0);
        r1 = mfma4(Ar1[r], Bv[r], r1);
      }
    }
  }
}

// Step-0 gate table (encoder_layout.h: G0Header): one wave per 16 consecutive atom ids, fed exactly like a tile of the atom
// phase - lane (a, q) holds atom_table[a0 + a][4 q ..] and [16 + 4 q ..], zeros for a0 + a >= Va (column Va is the zero
// row: computed, not copied from the bias, so a non-finite weight gives the 0 * inf = NaN the atom phase gives) - with
// step 0's update image read from the prepared buffer.  G0[a] = z 0..31, r 0..31.
template <bool X3>
__global__ __launch_bounds__(64) void typed_g0_kernel(const float* upd0, const float* atom_table, float* g0, G0Header* hdr,
                                                      int Va, int Vb, int S) {
  const int lane = threadIdx.x, a = lane & 15, q = lane >> 4;
  const int ai = 16 * blockIdx.x + a;
  f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = h0;
  if (ai < Va) {
    h0 = ld4(atom_table + (size_t)ai * kD + 4 * q);
    h1 = ld4(atom_table + (size_t)ai * kD + 16 + 4 * q);
  }
  f32x4 z0, z1, r0, r1;
  gates_h_half<X3>(upd0, upd0 + (X3 ? kXVecFloatOff : kTVecFloatOff), lane, q, h0, h1, z0, z1, r0, r1);
  if (ai <= Va) {
    float* row = g0 + (size_t)ai * kG0Row + 4 * q;
    st4(row, z0);
    st4(row + 16, z1);
    st4(row + 32, r0);
    st4(row + 48, r1);
  }
  if (blockIdx.x == 0 && lane == 0) *hdr = G0Header{kG0Magic, Va, Vb, S};
}

// Which of the two step-0 savings an instantiation takes (diagnostics builds may switch either off):
//   IMPNN_T_G0     the z / r accumulators of a step-0 tile start from the gate table instead of bias + W_h h
//   IMPNN_T_POOLB  the pool reads a molecule's row indices, then its rows, five at a time
#ifndef IMPNN_T_G0
#define IMPNN_T_G0 1
#endif
#ifndef IMPNN_T_POOLB
#define IMPNN_T_POOLB 1
#endif
constexpr bool kUseG0 = IMPNN_T_G0 != 0, kPoolBatch = IMPNN_T_POOLB != 0;
// The start of a table-fed chunk - one whose ion's image carries both tables.  IMPNN_T_PEEL is on; IMPNN_T_REC2 and
// IMPNN_T_IMGH were measured and dropped and are off: each made the kernel slower than the peel alone.
//   IMPNN_T_PEEL   step 0 leaves the step loop: its tile's h rows and Reduce's record words are requested in front of
//                  the prologue barrier, nothing fills h, and the mid-step barrier of that step is gone
#ifndef IMPNN_T_PEEL
#define IMPNN_T_PEEL 1
#endif
// (Measured and dropped, DESIGN.md 4.1: the tile's G0 rows among those pre-loads, and the scalar chain of the wave's two fixed
//  runs in front of that barrier too - the transfers of fetch_step0 have landed when the prologue barrier is reached, so what
//  is requested in front of it is waited for in full, by all sixteen waves.)
//   IMPNN_T_REC2   a launch in which every ion is table-fed keeps TWO record buffers, the second where the LDS copy of
//                  the atom table lay (nothing but fill_h0 read it): the next chunk's record is stored into the idle one
//                  behind step 0, so the store behind the pool and its barrier are gone
//   IMPNN_T_IMGH   fetch_step0 leaves the h-half blocks of z and r out of step 0's update image when the chunk's ion has
//                  the gate table: step 0 never reads them (mode 3: 12 of the image's 37 one-KB granules)
#ifndef IMPNN_T_REC2
#define IMPNN_T_REC2 0
#endif
#ifndef IMPNN_T_IMGH
#define IMPNN_T_IMGH 0
#endif
constexpr bool kPeel = kUseG0 && IMPNN_T_PEEL != 0, kTwoRec = kPeel && IMPNN_T_REC2 != 0;
constexpr bool kSkipImgH = kUseG0 && IMPNN_T_IMGH != 0;

// Where the loads of the NEXT step are issued (diagnostics builds may override):
//   kPfWhere   0: the step's update image at the top of its own message phase; 1: during the previous step's atom phase,
//              in front of the GEMMs; 2: behind the GEMMs (registers are free there, the vector-memory path still idle)
//   kRunsEarly how many of a wave's two fixed type runs (0-2) have their matrix rows requested in front of the previous
//              step's GEMMs (16 VGPRs each through the GEMMs); the others at the top of the message phase
#ifndef IMPNN_T_PF
#define IMPNN_T_PF 0
#endif
#ifndef IMPNN_T_EARLY
#define IMPNN_T_EARLY 0
#endif
constexpr int kPfWhere = IMPNN_T_PF, kRunsEarly = IMPNN_T_EARLY;
// Reduce (models/layers.py:57-83), the in-edge ranks d0 .. d0 + N - 1 of a tile's rows in one LDS round trip: agg += the
// rows' messages of these ranks, in rank order; a rank a row does not have reads the slot of zeros (x + 0 = x: no branch,
// all 2 N loads of the round in flight together).  jd: the four u16 of the record's jdptr at d0 (u16[260] incl. padding,
// d0 a multiple of 4: one aligned 8-byte read, d0 + 3 <= 258).
// LANES: the adds as single-lane instructions (mode 3 runs them beside the MFMAs
// of the gates' h halves, where a v_pk_add_f32 costs more issue time than two v_add_f32; the same IEEE sums either way).
template <int N, bool LANES>
__device__ __forceinline__ void reduce_ranks(const float* msg, const uint2 jd, int d0, int deg, int row, int q,
                                             int zero_slot, f32x4& agg0, f32x4& agg1) {
  const int first[4] = {(int)(jd.x & 0xffffu), (int)(jd.x >> 16), (int)(jd.y & 0xffffu), (int)(jd.y >> 16)};
  f32x4 m0v[N], m1v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int o = tmsg_off(d0 + j < deg ? first[j] + row : zero_slot, q);
    m0v[j] = ld4(msg + o);
    m1v[j] = ld4(msg + (o ^ 16));  // unit 4 + q of the same slot
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if constexpr (LANES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        agg0[i] = lane1(agg0[i] + m0v[j][i]);
        agg1[i] = lane1(agg1[i] + m1v[j][i]);
      }
    } else {
      agg0 += m0v[j];
      agg1 += m1v[j];
    }
  }
}

// One statement of quad arithmetic for both instruction forms: quad<false>(f, a...) is f on whole quads (packed f32
// instructions), quad<true> applies f element by element, and keep1 - lane1 for a single element, nothing for a quad -
// marks the results that stay in registers of their own, so that the elements are not paired up again.
__device__ __forceinline__ float keep1(float v) { return lane1(v); }
__device__ __forceinline__ f32x4 keep1(f32x4 v) { return v; }
template <bool LANES, class F, class... A>
__device__ __forceinline__ f32x4 quad(F f, A... a) {
  if constexpr (LANES) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = f(a[i]...);
    return r;
  } else {
    return f(a...);
  }
}

// What a tile's wave holds of step 0 of a table-fed chunk when it leaves the prologue barrier (lane (a, q) of row a): the
// row's h quads and Reduce's first record words.
struct Step0Pre {
  f32x4 h0, h1;
  uint2 jd;
  int deg, maxdeg;
};

template <bool STAMPS, bool X3, int HS = kTHS>
__global__ __launch_bounds__(kThreads, kThreads / 256) void encoder_typed_kernel(TEncParams p) {
  extern __shared__ __align__(16) float smem[];
  constexpr int kUpdLds = X3 ? kXUpdLds : kTUpdLds, kUpdSlot = X3 ? kXUpdSlot : kTUpdSlot;
  constexpr int kNPf = X3 ? 3 : 2;  // 16-byte loads per thread that carry one update image
  float* const wupd = smem + kOffUpd;
  float* const wvec = wupd + (X3 ? kXVecFloatOff : kTVecFloatOff);
  float* const hbuf = smem + off_h(X3);
  float* const msg = smem + off_msg(X3, HS);
  const int zero_slot = p.ecap + 1;  // (dump slot: p.ecap)
  // The record buffer of the current chunk: recl0, or - two record buffers (kTwoRec, below) - recl0 + rec_lds in turn.
  unsigned char* const recl0 = reinterpret_cast<unsigned char*>(smem + off_rec(X3, p.ecap, HS));
  const int rec_lds = p.rec_lds;                                  // trec_lds_bytes(Vb)
  float* const atab = reinterpret_cast<float*>(recl0 + rec_lds);  // Va rows + one zero row (when it fits)
  unsigned char* recl;
  const uint16_t *r_rowdeg, *r_moloff, *r_molrows, *r_poolrow, *r_jdptr, *r_runs;
  const unsigned char* r_tilemax;
  const int32_t* r_rowatom;
  int* run_ctr;  // next dynamically assigned type run
  const uint4* r_grp;
  const uint32_t* grp_x;
  auto use_record = [&](unsigned char* base) {
    recl = base;
    r_rowdeg = reinterpret_cast<const uint16_t*>(recl + kTRecRowdeg);
    r_tilemax = recl + kTRecTilemax;
    r_moloff = reinterpret_cast<const uint16_t*>(recl + kTRecMoloff);
    r_molrows = reinterpret_cast<const uint16_t*>(recl + kTRecMolrows);
    r_poolrow = reinterpret_cast<const uint16_t*>(recl + kTRecPoolrow);
    r_rowatom = reinterpret_cast<const int32_t*>(recl + kTRecRowatom);
    r_jdptr = reinterpret_cast<const uint16_t*>(recl + kTRecJdptr);
    r_runs = reinterpret_cast<const uint16_t*>(recl + trec_runs_off(p.Vb, p.ecap));
    run_ctr = reinterpret_cast<int*>(recl + kTRecCounts + 8);
    r_grp = reinterpret_cast<const uint4*>(recl + kTRecGrp);
    grp_x = reinterpret_cast<const uint32_t*>(r_grp);
  };
  use_record(recl0);

  const int tid = threadIdx.x, lane = tid & 63;
  // (readfirstlane: uniform to the compiler too, so the run loop's conditions stay scalar - and no register spills)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, q = lane >> 4;
  // diagnostics build only (impnn_debug_set_stamp_buffer): the stamp bookkeeping costs ~10 VGPRs
  unsigned long long* stamp = STAMPS && p.stamps ? p.stamps + (size_t)blockIdx.x * 32 : nullptr;
  if (stamp && tid == 0) stamp[0] = __builtin_amdgcn_s_memtime();

  // The workspace must hold a typed plan made for this launch geometry (impnn_encoder_plan with the same
  // arguments): anything else would be read at wrong offsets.  A mismatch - or a batch the plan found it cannot
  // cut into chunks (PlanHeader::overflow) - poisons the outputs instead.
  {
    const PlanHeader hd = *p.header;
    if (hd.magic != kPlanMagic || hd.kind != 1 || hd.nwg != (int)gridDim.x || hd.max_sub != p.max_sub ||
        hd.B != p.B || hd.n_ions != p.n_ions || hd.overflow != 0) {
      const float nan = __builtin_nanf("");
      for (int g = 0; g < p.n_ions; ++g)
        for (int64_t t = (int64_t)blockIdx.x * kThreads + tid; t < (int64_t)p.B * kD; t += (int64_t)gridDim.x * kThreads)
          p.pooled[g][t] = nan;
      return;
    }
  }
  const int c_begin = blockIdx.x * p.max_sub;
  const int c_end = c_begin + __builtin_amdgcn_readfirstlane(p.nsub[blockIdx.x]);
  if (c_begin >= c_end) return;

  bool atab_in_lds = p.atab_lds;  // (false as well where the second record buffer takes its place: below)
  auto copy_atab = [&]() {
    for (int t = tid; t < (p.Va + 1) * (kTAS / 4); t += kThreads)  // kTAS == kD: a verbatim copy + one zero row
      st4(atab + 4 * t, t < p.Va * (kD / 4) ? ld4(p.atom_table + 4 * t) : f32x4{0.f, 0.f, 0.f, 0.f});
  };
  if (p.atab_lds && p.S == 0) copy_atab();
  if (tid < kD) msg[zero_slot * kD + tid] = 0.f;  // never written again: what a row reads beyond its in-degree
  unsigned long long t_pro = 0, t_steps = 0, t_pool = 0, t_mark = 0, t_msg = 0;
  if (stamp && tid == 0) t_mark = __builtin_amdgcn_s_memtime();

  // ---- GlobalSumPool (models/layers.py:161-164), as in encoder_fused.hip: eight lanes share one
  //      (molecule, 4 features), ascending rows, then a fixed 3-step butterfly on the DPP network.
  auto pool = [&](int M, int m0, int g) {
    float* out_g = p.pooled[g];
    for (int t0 = 0; t0 < M * 64; t0 += kThreads) {
      const int t = t0 + tid;
      const int part = t & 7, f4 = (t >> 3) & 7, m = t >> 6;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        const int nr = r_molrows[m], mo = r_moloff[m];
        if constexpr (kPoolBatch) {
          // Five of the lane's rows per turn (a molecule of <= 40 rows: one turn): their indices in one LDS round trip,
          // the rows in a second, then the adds in ascending n - not two dependent round trips per row.  A row that is
          // not pooled, or lies beyond the molecule, adds +0 instead of nothing: acc starts at +0 and no sum of it is
          // -0, so x + 0 = x holds for every value it takes - the same bits.  (All loads unconditional: index 0 and
          // row 0 where there is nothing to read.)
          constexpr int kPB5 = 5;
          for (int n0 = part; n0 < nr; n0 += 8 * kPB5) {
            int pr[kPB5];
#pragma unroll
            for (int j = 0; j < kPB5; ++j) {
              const int n = n0 + 8 * j;
              const int w = r_poolrow[n < nr ? mo + n : 0];
              pr[j] = n < nr ? w : 0;
            }
            f32x4 v[kPB5];
#pragma unroll
            for (int j = 0; j < kPB5; ++j) v[j] = ld4(hbuf + (pr[j] & 0xff) * HS + 4 * f4);
#pragma unroll
            for (int j = 0; j < kPB5; ++j) acc += (pr[j] & 0x8000) ? v[j] : f32x4{0.f, 0.f, 0.f, 0.f};
          }
        } else {
          for (int n = part; n < nr; n += 8) {
            const int pr = r_poolrow[mo + n];
            if (pr & 0x8000) acc += ld4(hbuf + (pr & 0xff) * HS + 4 * f4);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = acc[i];
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, true));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, true));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));
        acc[i] = v;
      }
      if (m < M && part == 0) st4(out_g + (int64_t)(m0 + m) * kD + 4 * f4, acc);
    }
  };
  // h0 = atom_table[atom id of the placed row]: 4 threads per row, 2 x 16 B each; slack rows: zeros.  From the LDS copy of
  // the table when there is one: step 0 then reads h like every other step (no per-group branch, a compile-time stride).
  auto fill_h0 = [&]() {
    const int row = tid >> 2, sub = tid & 3;
    const int id = r_rowatom[row];
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if ((unsigned)id < (unsigned)p.Va) {
      if (atab_in_lds) {
        v0 = ld4(atab + id * kTAS + 8 * sub);
        v1 = ld4(atab + id * kTAS + 8 * sub + 4);
      } else {
        // (an opaque copy of the lane's part: the 64-bit address atom_table + 8 sub would otherwise be kept - spilled -
        //  through the whole kernel for this cold path)
        int sb = sub;
        asm volatile("" : "+v"(sb));
        v0 = ld4(p.atom_table + (int64_t)id * kD + 8 * sb);
        v1 = ld4(p.atom_table + (int64_t)id * kD + 8 * sb + 4);
      }
    }
    st4(hbuf + row * HS + 8 * sub, v0);
    st4(hbuf + row * HS + 8 * sub + 4, v1);
  };

  if (p.S == 0) {  // no message passing: pooled = GlobalSumPool(Embedding(atom ids)); kept apart from the step machinery
    for (int c = c_begin; c < c_end; ++c) {
      const unsigned char* rc = p.rec + (size_t)c * kTRecBytes;
      if (8 * tid < rec_lds) reinterpret_cast<uint2*>(recl)[tid] = reinterpret_cast<const uint2*>(rc)[tid];
      const int4 dsc = reinterpret_cast<const int4*>(p.desc)[c];
      lds_barrier();
      fill_h0();
      lds_barrier();
      pool(__builtin_amdgcn_readfirstlane(dsc.y), __builtin_amdgcn_readfirstlane(dsc.x),
           __builtin_amdgcn_readfirstlane(dsc.w) >> 16);
      lds_barrier();
    }
    return;
  }

  // Step-0 message table: one uniform read of each ion's image header.  An image without a table (the plain prepare
  // entry, the per-call rebuild) or one built for other vocabularies takes the MFMA path below, unchanged.
  unsigned tabmask = 0;
  {
    const M0Header t0 = *reinterpret_cast<const M0Header*>(p.upd[0] + kUpdLds);
    if (t0.magic == kM0Magic && t0.Va == p.Va && t0.Vb == p.Vb && t0.S == p.S) tabmask |= 1u;
    if (p.n_ions > 1) {
      const M0Header t1 = *reinterpret_cast<const M0Header*>(p.upd[1] + kUpdLds);
      if (t1.magic == kM0Magic && t1.Va == p.Va && t1.Vb == p.Vb && t1.S == p.S) tabmask |= 2u;
    }
  }
  // Step-0 gate table: only behind a message table that is in use, and only if the second header agrees (an image of the
  // with-atoms entry or any older one holds zeros there).
  // Bits 2 and 3 of the same word (the kernel has no scalar register to spare for a second one).
  if constexpr (kUseG0) {
    for (int g = 0; g < p.n_ions; ++g) {
      if (!((tabmask >> g) & 1u)) continue;
      const G0Header t = *reinterpret_cast<const G0Header*>(p.upd[g] + kUpdLds + kG0HeaderFloatOff);
      if (t.magic == kG0Magic && t.Va == p.Va && t.Vb == p.Vb && t.S == p.S) tabmask |= 4u << g;
    }
  }

  // Two record buffers: every ion of the launch table-fed (so every chunk is peeled and nothing but the pre-loads reads the
  // atom table - they take it from L2 then, with fill_h0's select), and a second record fits where the host made room for
  // the LDS copy of the table.  Workgroup-uniform.  The buffers alternate chunk by chunk; the next chunk's record reaches
  // the idle one from the registers it travels in, behind step 0's end-of-step barrier (its loads were requested a whole
  // atom phase earlier; the idle buffer's last readers were the previous chunk's pool, in front of that pool's barrier).
  bool two_rec = false;
  if constexpr (kTwoRec)
    two_rec = p.atab_lds && tabmask == (p.n_ions > 1 ? 0xfu : 0x5u) && rec_lds <= (p.Va + 1) * kTAS * (int)sizeof(float);
  if (two_rec) atab_in_lds = false;
  if (atab_in_lds) copy_atab();
  bool rec_in_lds = false;  // the current chunk's record is in its buffer already

  // The record of the NEXT chunk travels in registers while the current chunk runs.
  const bool rec_big = rec_lds > kTRecPart1;  // workgroup-uniform
  const unsigned char* rec_c = p.rec + (size_t)c_begin * kTRecBytes;
  uint2 rec_n8 = reinterpret_cast<const uint2*>(rec_c)[tid];
  uint32_t rec_n4 = rec_big ? reinterpret_cast<const uint32_t*>(rec_c + kTRecPart1)[tid] : 0u;
  int4 dsc_next = reinterpret_cast<const int4*>(p.desc)[c_begin];

  // ---- Step 0's inputs of chunk `cn` (descriptor dn), global -> LDS without a register in between (glds16):
  //   * step 0's update image of the chunk's ion -> wupd, 64 units of 16 bytes per instruction;
  //   * if that ion's image carries the table: the chunk's step-0 messages -> msg.  The valid message slots are dense in
  //     [0, edges) and a slot is 128 contiguous bytes, so one instruction fills the eight slots base .. base + 7: lane l
  //     copies, for slot s = base + (l >> 3), the unit that tmsg_off places at position l & 7 of the slot, out of row
  //     M0[type][min(id, Va)] - type and id from the plan's slot-ordered list (encoder_layout.h: tsrc_word).  Slots at
  //     and beyond `edges` (the list holds nothing there: never read) copy row 0 into slots nothing reads; edges <= ecap
  //     and ecap is a multiple of 8, so the rounding reaches neither the dump slot nor the slot of zeros.
  // Called where nothing reads or writes msg and wupd - the kernel preamble, and behind the end-of-step barrier of a
  // chunk's last step - so the transfers fly under the pool and the record copy; the prologue barrier in front of step 0
  // waits for them (vmcnt(0)).  `dn` must be cn's descriptor: the table bit is the NEXT chunk's ion's.
  auto fetch_step0 = [&](const int4 dn, int cn) {
    const int gn = __builtin_amdgcn_readfirstlane(dn.w) >> 16;
    const float* const ug = p.upd[gn];
    static_assert(kUpdLds % 256 == 0, "whole 64-lane transfers");
    // (the lane and wave roles are derived here, behind opaque copies of the two ids: hoisted out of the chunk loop they
    //  would occupy registers - vector and scalar - through the whole kernel, which has none to spare)
    int ln = lane, wv = wave;
    asm volatile("" : "+v"(ln), "+s"(wv));
    const bool tabn = (tabmask >> gn) & 1u;  // workgroup-uniform
    int edges = __builtin_amdgcn_readfirstlane(dn.z);
    edges = tabn ? (edges < p.ecap ? edges : p.ecap) : 0;
    constexpr int kIt = (kTECapBig / 8 + kWaves - 1) / kWaves;  // granules per wave at most
    // All list words first: one round trip, not one per granule.  Unconditional loads (a clamped address inside the
    // chunk's list; the word is dropped where the slot is not in use), all of them landed in front of the first message
    // transfer (the empty asm below): nothing the compiler knows of is then in flight behind this lambda, so it places
    // no s_waitcnt of its own - which would wait for the transfers as well - in front of the pool.
    uint32_t sw[kIt];
    if (tabn) {
      const uint32_t* const lst = p.slist + (size_t)cn * p.ecap;
#pragma unroll
      for (int i = 0; i < kIt; ++i) {
        const int sl = 8 * (wv + i * kWaves) + (ln >> 3);
        const uint32_t word = lst[sl < edges ? sl : 0];
        sw[i] = sl < edges ? word : 0u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < kIt; ++i) sw[i] = 0u;
    }
    constexpr int kUIt = (kUpdLds / 256 + kWaves - 1) / kWaves;
    // (kSkipImgH: with the gate table in use, step 0 starts z and r behind their h half, so the blocks that multiply h -
    //  half 0 of the gates' blocks, image layout as in gates_h_half - are not sent; every later step stores its whole image)
    const bool gaten = kSkipImgH && ((tabmask >> (2 + gn)) & 1u);  // workgroup-uniform
#pragma unroll
    for (int i = 0; i < kUIt; ++i) {  // (under the list's round trip)
      const int gi = wv + i * kWaves, ub = 64 * gi;  // granule of 1 KB
      // mode 3: block ((gate*2 + T)*2 + half) is 3 granules; mode 2: block ((gate*2 + T)*2 + half)*2 + u is one
      const bool h_half = X3 ? (gi < 24 && ((gi / 3) & 1) == 0) : (gi < 16 && (gi & 2) == 0);
      if (ub < kUpdLds / 4 && !(gaten && h_half)) glds16(ug + 4 * (ub + ln), wupd + 4 * ub);  // (wave-uniform)
    }
    static_assert(kIt == 5, "the list words are landed by name");
    asm volatile("" : "+v"(sw[0]), "+v"(sw[1]), "+v"(sw[2]), "+v"(sw[3]), "+v"(sw[4]) : : "memory");
    const float* const m0_g = p.m0[gn];
#pragma unroll
    for (int i = 0; i < kIt; ++i) {
      const int base = 8 * (wv + i * kWaves);
      if (base < edges) {  // (wave-uniform)
        const int sl = base + (ln >> 3);
        const unsigned type = min(sw[i] >> 24, (unsigned)p.Vb - 1u), col = min(sw[i] & kSrcIdNone, (unsigned)p.Va);
        const unsigned off = (type * (unsigned)(p.Va + 1) + col) * kD + 4u * ((ln & 7) ^ ((sl >> 1) & 7));  // the table is < 2 MiB
        glds16(m0_g + off, msg + kD * base);
      }
    }
  };
  fetch_step0(dsc_next, c_begin);

  // message-phase lane roles (see the message phase below)
  const int kh = lane >> 5, f = lane & 31;
  const int boff = kh * 512 + f * 4;
  const int ysh = 8 * (lane & 3), zsh = 16 * kh;
  const int acol = 16 * kh + 2 * ((lane >> 2) & 7);  // first of the two h columns this lane feeds (see Grp)

  for (int c = c_begin; c < c_end; ++c) {
    // ---- chunk prologue: descriptor, record -> LDS, h0 = atom_table[atom ids]
    const int4 dsc = dsc_next;
    const int m0 = __builtin_amdgcn_readfirstlane(dsc.x), M = __builtin_amdgcn_readfirstlane(dsc.y);
    const int rg = __builtin_amdgcn_readfirstlane(dsc.w);
    const int R = rg & 0xffff, g = rg >> 16;
    const int ntiles = (R + 15) >> 4;
    const float* upd_g = p.upd[g];
    const float* tmat_g = p.tmat[g];
    const bool tab0 = (tabmask >> g) & 1u;  // workgroup-uniform: step 0's messages come from the table
    auto store_record = [&](unsigned char* dst) {
      if (8 * tid < rec_lds) reinterpret_cast<uint2*>(dst)[tid] = rec_n8;
      if (rec_big && kTRecPart1 + 4 * tid < rec_lds) reinterpret_cast<uint32_t*>(dst + kTRecPart1)[tid] = rec_n4;
    };
    if (!rec_in_lds) {
      store_record(recl);
      lds_barrier();
    }
    // A table-fed chunk (both tables): step 0 has no message phase and takes the h half of its gates from G0, so nothing
    // reads h in that step but lane (a, q) its own row's quads - for r h, the blend and the residual.  Those go straight
    // into the registers of the tile's wave, with Reduce's record words, HERE: every register of the message phase is
    // free, and the LDS round trips pass in front of the prologue barrier.  No fill_h0 - 1024 threads, five LDS accesses
    // each in a chain three deep - and step 0 runs outside the step loop (below), without a mid-step barrier.  Rows of
    // hbuf that belong to no tile of this chunk keep the previous chunk's bytes; nothing reads them.
    const bool peel = kPeel && ((tabmask >> g) & 1u) && ((tabmask >> (2 + g)) & 1u);  // workgroup-uniform
    // Tile -> wave map as in encoder_fused.hip: waves w, w+4, w+8, w+12 share a SIMD; tiles are ordered heavy -> light,
    // the SIMD groups with one tile fewer take the heaviest.  (Evaluated where it is asked: no register held for it.)
    auto tile_of_wave = [&](const int wave) -> int {
      int my_tile = -1;
      const int grp = wave & 3, slot = wave >> 2, q4 = ntiles >> 2, r4 = ntiles & 3;
      const int heavy = (4 - r4) * q4;
      if (grp >= r4) {
        if (slot < q4) my_tile = slot * (4 - r4) + (grp - r4);
      } else if (slot <= q4) {
        my_tile = heavy + slot * r4 + grp;
      }
      return my_tile < ntiles ? my_tile : -1;
    };
    // (Given a value on every path: left undefined for the waves without a tile, the compiler keeps five of the quads in
    //  scratch between the two places - 100-120 bytes in every instantiation.)
    Step0Pre pre{};
    auto preload_step0 = [&]() {
      // (lane and wave roles from opaque copies of the ids, as in fetch_step0: shared with the step loop's atom phase they
      //  would be held in registers through every message phase)
      int ln = lane, wv = wave;
      asm volatile("" : "+v"(ln), "+s"(wv));
      const int a = ln & 15, q = ln >> 4;
      const int tile = tile_of_wave(wv);
      if (tile >= 0) {
        const int row = tile * 16 + a;
        const int id = r_rowatom[row];
        pre.deg = r_rowdeg[row];
        pre.maxdeg = r_tilemax[tile];
        pre.jd = *reinterpret_cast<const uint2*>(r_jdptr);
        // (clamped exactly where fill_h0 writes zeros: the zero row of the LDS atom table)
        const unsigned col = (unsigned)id < (unsigned)p.Va ? (unsigned)id : (unsigned)p.Va;
        if (atab_in_lds) {
          pre.h0 = ld4(atab + col * kTAS + 4 * q);
          pre.h1 = ld4(atab + col * kTAS + 16 + 4 * q);
        } else {
          pre.h0 = pre.h1 = f32x4{0.f, 0.f, 0.f, 0.f};
          if ((unsigned)id < (unsigned)p.Va) {
            pre.h0 = ld4(p.atom_table + (int64_t)id * kD + 4 * q);
            pre.h1 = ld4(p.atom_table + (int64_t)id * kD + 16 + 4 * q);
          }
        }
      }
    };
    if (peel)
      preload_step0();
    else
      fill_h0();
    // (step 0's messages - when the image carries the table - and its update image are on their way into LDS since the
    //  previous chunk's last step: fetch_step0)
    if (tid == 0) *run_ctr = 2 * kWaves;  // runs 0 .. 2 kWaves - 1 are assigned statically (two per wave)
    // Prologue barrier: h0 is in place - and so is everything fetch_step0 sent on its way: every wave waits for its own
    // transfers (vmcnt(0), explicitly: the compiler does not know of them - glds16), the barrier then publishes them to
    // the others.
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    {  // the record of the next chunk (behind the wait above, so that it does not wait for these loads as well)
      const int cn = (c + 1) < c_end ? (c + 1) : c;  // clamped: unconditional loads
      const unsigned char* rn = p.rec + (size_t)cn * kTRecBytes;
      rec_n8 = reinterpret_cast<const uint2*>(rn)[tid];
      if (rec_big) rec_n4 = reinterpret_cast<const uint32_t*>(rn + kTRecPart1)[tid];
      dsc_next = reinterpret_cast<const int4*>(p.desc)[cn];
    }
    if (stamp && tid == 0) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      t_pro += t - t_mark;
      t_mark = t;
    }
    const int nrun = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const uint16_t*>(recl + kTRecNrun));

    // Two type runs per wave are in flight at any time (P, Q).  The first two of every step are fixed - runs `wave` and
    // `wave + 16` of the chunk's run table, the same in all S steps - so their group range and bond type are resolved
    // once per chunk, and their matrix rows for step s + 1 are requested during step s's atom phase, in
    // front of the GEMMs: the vector-memory path, which bounds the message phase (~280 KB of matrix rows per chunk-step
    // through one CU's L2 port), has nothing else to do there.  The step's update image travels the same way.
    Run P, Q;
    int gP = 0, nP = 0, gQ = 0, nQ = 0;
    bool haveP = false, haveQ = false;
    const bool sP = wave < nrun, sQ = wave + kWaves < nrun;
    const int sgP = __builtin_amdgcn_readfirstlane(r_runs[sP ? wave : 0]);
    const int snP = __builtin_amdgcn_readfirstlane(r_runs[(sP ? wave : 0) + 1]) - sgP;
    const int sgQ = __builtin_amdgcn_readfirstlane(r_runs[sQ ? wave + kWaves : 0]);
    const int snQ = __builtin_amdgcn_readfirstlane(r_runs[(sQ ? wave + kWaves : 0) + 1]) - sgQ;
    // (matrix offset of the run's type; `have` false: four cache lines of type 0 that nobody uses - see `fetch`)
    const int soP = sP ? (__builtin_amdgcn_readfirstlane(grp_x[4 * sgP]) & 0xff) * kTMatFloats : 0;
    const int soQ = sQ ? (__builtin_amdgcn_readfirstlane(grp_x[4 * sgQ]) & 0xff) * kTMatFloats : 0;
    const int lboffP = sP ? boff : 0, lboffQ = sQ ? boff : 0;
    f32x4 pf[kNPf];
    auto fetch_pf = [&](int s_) {  // update image of step s_
#pragma unroll
      for (int i = 0; i < kNPf; ++i) pf[i] = ld4(upd_g + (int64_t)s_ * kUpdSlot + 4 * (tid + i * kThreads));
    };
    auto fetch_P = [&](int s_) {  // matrix rows of the wave's first / second fixed run in step s_
      const float* tm = tmat_g + (size_t)s_ * p.Vb * kTMatFloats;
#pragma unroll
      for (int i = 0; i < 4; ++i) P.bq[i] = ld4(tm + soP + lboffP + i * 128);
    };
    auto fetch_Q = [&](int s_) {
      const float* tm = tmat_g + (size_t)s_ * p.Vb * kTMatFloats;
#pragma unroll
      for (int i = 0; i < 4; ++i) Q.bq[i] = ld4(tm + soQ + lboffQ + i * 128);
    };
    // step 0: what later steps request during the previous atom phase is requested here (its update image is in LDS)
    if (kRunsEarly >= 1) fetch_P(0);
    if (kRunsEarly >= 2) fetch_Q(0);
    // ---- atom phase: one 16-atom tile per wave (tile_of_wave above), for step s.  Stated once and instantiated twice:
    // FIRST = step 0 of a table-fed chunk, outside the step loop - the rows' h quads and Reduce's record words are in `pre`
    // (requested in front of the prologue barrier), so nothing is live around the loop's back edge for it, and the z / r
    // accumulators start from G0 without a branch; otherwise a step of the loop.
    auto atom_phase = [&](auto first_step, const int s) {
      constexpr bool FIRST = decltype(first_step)::value;
      const bool mstamp = !FIRST && stamp && c == c_begin && s == 1;
      // (FIRST: lane and wave roles from opaque copies of the ids, so that nothing it derives from them is shared with - and
      //  held in registers for - the instantiation inside the step loop)
      int ln = lane, wv = wave;
      if constexpr (FIRST) asm volatile("" : "+v"(ln), "+s"(wv));
      const int lane = ln, wave = wv, a = ln & 15, q = ln >> 4;
      const int my_tile = tile_of_wave(wave);
      const bool has_tile = my_tile >= 0;
      if (has_tile) {
        const int tile = my_tile;
        const int row = tile * 16 + a;
        const int deg = FIRST ? pre.deg : (int)r_rowdeg[row];
        const int maxdeg = __builtin_amdgcn_readfirstlane(FIRST ? pre.maxdeg : (int)r_tilemax[tile]);
        // ---- gates z, r (models/layers.py:144-147) and candidate (:150-151): out^T = W^T [h | agg]^T.  z and r accumulate
        // bias, then W_h h, then W_agg agg; the first half needs no message.  Mode 3 issues it HERE, in front of Reduce: the
        // bf16 pipe co-executes with the vector ALU and the LDS, so Reduce's round trips pass under these 36 MFMAs - and with
        // the h halves out of the way the gates' single-lane arithmetic below fits the registers (without this order it
        // spills 8 bytes).  The order of every sum is unchanged.  (The exact-f32 MFMA shares the issue port with the
        // vector ALU: nothing passes under it, and reads of h in front of Reduce alone cost time - DESIGN.md 4.1.)
        // Step 0 of an ion whose image carries the gate table: h is atom_table[id] or zeros, so bias + W_h h is row
        // min(id, Va) of G0 (clamped exactly where fill_h0 writes zeros) - four 16-byte loads from L2, requested here so
        // that they pass under Reduce and land, in the accumulators themselves, where the agg half starts.  No bias
        // read, no split of h, none of the h half's MFMAs; h itself is still read, for r * h and the blend.
        // FIRST: h is in `pre` already - no read of the h buffer (nothing filled it) - and the gate table is taken for granted.
        f32x4 h0, h1, z0, z1, r0, r1;
        if constexpr (FIRST) h0 = pre.h0, h1 = pre.h1;
        // (workgroup-uniform; evaluated where it is asked, from an opaque copy of the mask: as a value of the chunk the
        //  compiler keeps it - and the table's address - in scalar registers over all steps, and the kernel has none left:
        //  what it spills there costs vector registers)
        auto gate_tab = [&]() -> bool {
          if constexpr (!kUseG0 || kPeel) return false;  // (kPeel: every chunk with the gate bit takes FIRST)
          unsigned tm = tabmask;
          asm volatile("" : "+s"(tm));
          return s == 0 && ((tm >> (2 + g)) & 1u);
        };
        auto load_gates = [&]() {
          const int id = r_rowatom[row];
          const unsigned col = (unsigned)id < (unsigned)p.Va ? (unsigned)id : (unsigned)p.Va;
          // (the table's address is read here, through an opaque copy of the ion: held over the chunk it would cost the
          //  scalar registers the kernel does not have)
          int gg = g;
          asm volatile("" : "+s"(gg));
          // (a 32-bit byte offset beside the scalar base - the table is < 4 MiB / Vb: one address register, not two)
          const unsigned boff = col * (unsigned)(kG0Row * sizeof(float)) + 16u * (unsigned)q;
          const float* const gp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.g0[gg]) + boff);
          z0 = ld4(gp), z1 = ld4(gp + 16);
          r0 = ld4(gp + 32), r1 = ld4(gp + 48);
        };
        // (mode 3's A operands: block ((gate*2 + T)*2 + half) of the image, 3 x 512 bf16)
        [[maybe_unused]] const __bf16* const wb = reinterpret_cast<const __bf16*>(wupd);
        if constexpr (X3 && FIRST) {
          load_gates();
        } else if constexpr (X3) {
          h0 = ld4(hbuf + row * HS + 4 * q);
          h1 = ld4(hbuf + row * HS + 16 + 4 * q);
          if (gate_tab())
            load_gates();
          else
            gates_h_half<true>(wupd, wvec, lane, q, h0, h1, z0, z1, r0, r1);
        }
        // ---- Reduce: in-edge messages summed in edge-slot order, in the form the tile's largest in-degree (wave-uniform)
        // asks for: one rank per round trip, two, or a loop of four per round.  agg starts at +0 in every form, and what
        // the short forms leave out are adds of the slot of zeros (x + 0 = x for every x that a sum 0 + m can be, a first
        // message of -0 included): the same bits as the loop's.
        f32x4 agg0 = {0.f, 0.f, 0.f, 0.f}, agg1 = agg0;
        auto jd_at = [&](int d0) -> uint2 {  // (FIRST: the words of d0 = 0 came with `pre`)
          if constexpr (FIRST)
            if (d0 == 0) return pre.jd;
          return *reinterpret_cast<const uint2*>(r_jdptr + d0);
        };
        if (maxdeg <= 2) {
          if (maxdeg == 1) reduce_ranks<1, X3>(msg, jd_at(0), 0, deg, row, q, zero_slot, agg0, agg1);
          if (maxdeg == 2) reduce_ranks<2, X3>(msg, jd_at(0), 0, deg, row, q, zero_slot, agg0, agg1);
        } else {
          for (int d0 = 0; d0 < maxdeg; d0 += 4) reduce_ranks<4, X3>(msg, jd_at(d0), d0, deg, row, q, zero_slot, agg0, agg1);
        }
        if (mstamp && wave == 1 && lane == 0) stamp[8] = __builtin_amdgcn_s_memtime();
        // (Mode 3, measured and dropped: a static priority for two of a SIMD's four waves, so that they run ahead and the
        //  vector work of one pair overlaps the bf16 MFMAs of the other: +2 % kernel time - the waves that fall behind
        //  then set the length of the phase.)
        __builtin_amdgcn_s_setprio(1);
        if (s + 1 < p.S) {  // in flight under the GEMMs (see above)
          if (kPfWhere == 1) fetch_pf(s + 1);
          if (kRunsEarly >= 1) fetch_P(s + 1);
          if (kRunsEarly >= 2) fetch_Q(s + 1);
        }
        if constexpr (!X3 && FIRST) {
          load_gates();
        } else if constexpr (!X3) {
          h0 = ld4(hbuf + row * HS + 4 * q);
          h1 = ld4(hbuf + row * HS + 16 + 4 * q);
          // (mode 2 asks for its table rows only here: in front of Reduce the sixteen registers they land in are not
          //  free - the instantiation spilled 60 bytes - so their round trip is hidden by the SIMD's other waves alone)
          if (gate_tab())
            load_gates();
          else
            gates_h_half<false>(wupd, wvec, lane, q, h0, h1, z0, z1, r0, r1);
        }
        f32x4 t0 = ld4(wvec + 2 * kD + 4 * q), t1 = ld4(wvec + 2 * kD + 16 + 4 * q);
        if constexpr (X3) {
          // (Measured and dropped, DESIGN.md 4.1: the candidate's agg half in front of sigmoid(r), to run under the gate -
          //  no spill in this order, but +0.7 us per launch, and the sums of t change their order.)
          const B3 sa = split8x3(agg0, agg1);
          mma9x2(z0, z1, wb + ((0 * 2 + 0) * 2 + 1) * 1536, wb + ((0 * 2 + 1) * 2 + 1) * 1536, lane, sa);
          mma9x2(r0, r1, wb + ((1 * 2 + 0) * 2 + 1) * 1536, wb + ((1 * 2 + 1) * 2 + 1) * 1536, lane, sa);
          // the gates in single-lane instructions (encoder_device.h): the scheduler interleaves them with the MFMAs
          z0 = sigmoid4_lanes(z0);
          z1 = sigmoid4_lanes(z1);
          const f32x4 rh0 = mul4_lanes(sigmoid4_lanes(r0), h0);  // :149
          const f32x4 rh1 = mul4_lanes(sigmoid4_lanes(r1), h1);
          const B3 srh = split8x3(rh0, rh1);
          mma9x2(t0, t1, wb + ((2 * 2 + 0) * 2 + 0) * 1536, wb + ((2 * 2 + 1) * 2 + 0) * 1536, lane, srh);
          mma9x2(t0, t1, wb + ((2 * 2 + 0) * 2 + 1) * 1536, wb + ((2 * 2 + 1) * 2 + 1) * 1536, lane, sa);
        } else {
          // A operands: block ((gate*2 + T)*2 + half)*2 + u of the image, 16 B per lane, lane-linear (conflict-free)
          const float* wl = wupd + 4 * lane;
          // (the h half - the gate loop's half == 0 turns - ran above: gates_h_half, or the gate table)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int hu = 2 + u;
            const f32x4 Az0 = ld4(wl + ((0 * 2 + 0) * 4 + hu) * 256);
            const f32x4 Az1 = ld4(wl + ((0 * 2 + 1) * 4 + hu) * 256);
            const f32x4 Ar0 = ld4(wl + ((1 * 2 + 0) * 4 + hu) * 256);
            const f32x4 Ar1 = ld4(wl + ((1 * 2 + 1) * 4 + hu) * 256);
            const f32x4 Bv = u == 0 ? agg0 : agg1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              z0 = mfma4(Az0[r], Bv[r], z0);
              z1 = mfma4(Az1[r], Bv[r], z1);
              r0 = mfma4(Ar0[r], Bv[r], r0);
              r1 = mfma4(Ar1[r], Bv[r], r1);
            }
          }
          // (packed here: the f32 MFMA takes the vector ALU's issue slots, so what counts is the number of instructions -
          //  the single-lane forms were measured in this loop too: +1.8 us per launch)
          z0 = sigmoid4<false>(z0);
          z1 = sigmoid4<false>(z1);
          const f32x4 rh0 = sigmoid4<false>(r0) * h0;  // :149
          const f32x4 rh1 = sigmoid4<false>(r1) * h1;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int hu = half * 2 + u;
              const f32x4 Ah0 = ld4(wl + ((2 * 2 + 0) * 4 + hu) * 256);
              const f32x4 Ah1 = ld4(wl + ((2 * 2 + 1) * 4 + hu) * 256);
              const f32x4 Bv = half == 0 ? (u == 0 ? rh0 : rh1) : (u == 0 ? agg0 : agg1);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                t0 = mfma4(Ah0[r], Bv[r], t0);
                t1 = mfma4(Ah1[r], Bv[r], t1);
              }
            }
          }
        }
        __builtin_amdgcn_s_setprio(0);
        if (kPfWhere == 2 && s + 1 < p.S) {
          asm volatile("" ::: "memory");  // behind the GEMMs: their registers are free only now
          fetch_pf(s + 1);
        }
        if (mstamp && wave == 1 && lane == 0) stamp[9] = __builtin_amdgcn_s_memtime();
        // LayerNorm's gamma and beta are requested here, in front of the tanh: the GEMM operands are dead, so the
        // registers are free, and the round trip passes under the blend and the two cross-lane sums instead of behind the
        // v_rsq.  (sched_barrier: the scheduler otherwise sinks the four reads back down to their first use.)
        const f32x4 gm0 = ld4(wvec + 3 * kD + 4 * q), gm1 = ld4(wvec + 3 * kD + 16 + 4 * q);
        const f32x4 bt0 = ld4(wvec + 4 * kD + 4 * q), bt1 = ld4(wvec + 4 * kD + 16 + 4 * q);
        __builtin_amdgcn_sched_barrier(0);
        // ---- blend, LayerNorm, residual  (models/layers.py:153-155); (1-z) h + z t == h + z (t - h).
        // (The four feature quads of an atom sit in lanes l, l ^ 16, l ^ 32, l ^ 48; has_tile is wave-uniform, so EXEC is
        //  all ones here, which the lane swaps of sum_xor16_xor32 need.)
        // Stated once, for a quad in packed instructions or - mode 3 - element by element in single-lane instructions
        // (quad, keep1 above): a wave's epilogue runs beside the other three waves' bf16 MFMAs, and there the packed forms
        // cost the SIMD more issue time than they save; beside the exact-f32 MFMA they are the faster ones.
        const f32x4 th0 = X3 ? tanh4_lanes(t0) : tanh4<false>(t0), th1 = X3 ? tanh4_lanes(t1) : tanh4<false>(t1);
        const auto blend = [](auto z, auto th, auto h) { return keep1(z * (th - h) + h); };
        f32x4 n0 = quad<X3>(blend, z0, th0, h0), n1 = quad<X3>(blend, z1, th1, h1);
        const f32x4 s4 = quad<X3>([](auto x, auto y) { return keep1(x + y); }, n0, n1);
        const float sum = sum_xor16_xor32((s4[0] + s4[1]) + (s4[2] + s4[3]));
        const float mean = sum * (1.0f / kD);
        const auto center = [mean](auto n) { return keep1(n - mean); };
        n0 = quad<X3>(center, n0);
        n1 = quad<X3>(center, n1);
        const f32x4 q4 = quad<X3>([](auto x, auto y) { return keep1(x * x + y * y); }, n0, n1);
        const float var = sum_xor16_xor32((q4[0] + q4[1]) + (q4[2] + q4[3]));
        const float inv = __builtin_amdgcn_rsqf(var * (1.0f / kD) + p.ln_eps);
        const auto affine = [inv](auto n, auto gm, auto bt, auto h) { return keep1(n * keep1(gm * inv) + keep1(bt + h)); };
        const f32x4 o0 = quad<X3>(affine, n0, gm0, bt0, h0), o1 = quad<X3>(affine, n1, gm1, bt1, h1);
        st4(hbuf + row * HS + 4 * q, o0);
        st4(hbuf + row * HS + 16 + 4 * q, o1);
        if (mstamp && wave == 1 && lane == 0) stamp[10] = __builtin_amdgcn_s_memtime();
      }
      if (!has_tile && s + 1 < p.S) {  // waves without a tile in this chunk
        if (kPfWhere != 0) fetch_pf(s + 1);
        if (kRunsEarly >= 1) fetch_P(s + 1);
        if (kRunsEarly >= 2) fetch_Q(s + 1);
      }
      if (mstamp && wave == 1 && lane == 0) stamp[11] = __builtin_amdgcn_s_memtime();
    };
    if (stamp && c == c_begin && tid == 0) stamp[13] = __builtin_amdgcn_s_memtime();  // start of the first chunk's step 0
    if (peel) {  // step 0 of a table-fed chunk: the atom phase alone, then the end-of-step barrier
      __builtin_amdgcn_s_setprio(2);  // (as at the top of a step of the loop: Reduce ran at this priority in step 0 too)
      atom_phase(std::true_type{}, 0);
      lds_barrier();
      if (two_rec) {  // the next chunk's record -> the idle buffer; published by the barrier behind the pool
        store_record(recl == recl0 ? recl0 + rec_lds : recl0);
        rec_in_lds = true;
      }
      if (stamp && c == c_begin && tid == 0) stamp[14] = __builtin_amdgcn_s_memtime();
    }
    for (int s = peel ? 1 : 0; s < p.S; ++s) {
      const float* tm_s = tmat_g + (size_t)s * p.Vb * kTMatFloats;
      // ---- message phase: m_e = A[type_e] h[src_e], one group of <= 4 edges of one bond type per 16 MFMAs.
      // v_mfma_f32_4x4x1_16b: 16 independent 4x4 blocks.  Block b < 8 accumulates, for feature quad b, the k < 16
      // half of the dot products of the group's 4 edges; block 8 + b the k >= 16 half:
      //     D_b[i][j] += h[src_i][k] * A[type][4*(b & 7) + j][k],   k = 16*(b >> 3) + step.
      // The edge operand h[src_i][k] comes from ONE block per half-wave (lanes 0-3 / 32-35) and is broadcast to the
      // other seven by CBSZ/ABID: 8 lanes read LDS, not 64.  The matrix operand of lane l is half a row of A[type]
      // (16 floats = 4 x 16 B, straight from L2).  All groups of a type run on one wave, so a type's 4 KB are
      // fetched once per chunk-step.  The two k-halves meet in one v_permlane32_swap per edge pair; the sums go to
      // the LDS message buffer in jagged-diagonal order.
      // The f32 MFMA shares its issue port with the VALU (tools/ubench: no co-execution), so every VALU instruction in
      // this loop costs matrix time: the plan hands over ready-made LDS keys (message slot incl. swizzle; unused edge
      // lanes point at a dump slot, so the stores are unconditional) and the loop body is branch-free.
      __builtin_amdgcn_s_setprio(2);
      // (a step whose messages came from the table - fetch_step0 - requests no matrix rows and takes no run)
      const bool from_tab = tab0 && s == 0;  // workgroup-uniform
      if (kPfWhere == 0) {
        if (s > 0) {
          fetch_pf(s);
        } else {  // (defined on this path too: left as they are, the registers would stay live around the whole step loop)
#pragma unroll
          for (int i = 0; i < kNPf; ++i) pf[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      if (!from_tab) {
        const float* const abase = hbuf + acol;
        auto load_group = [&](int e, Grp& G) {
          G.ge = r_grp[e];
          const int src = __builtin_amdgcn_ubfe(G.ge.y, ysh, 8);
          G.aq = *reinterpret_cast<const f32x2v*>(abase + src * HS);
        };
        auto compute = [&](const Grp& G, const f32x4 (&bq)[4]) {
          float m01, m23;
          group_messages(G.aq, bq, m01, m23);
          msg[__builtin_amdgcn_ubfe(G.ge.z, zsh, 16) ^ f] = m01;
          msg[__builtin_amdgcn_ubfe(G.ge.w, zsh, 16) ^ f] = m23;
        };
        // A run's groups, software-pipelined: the operands of group e + 1 are requested from LDS in front of group e's
        // MFMAs (two buffers, loop unrolled by two so that neither is ever copied); the first group's were requested
        // when the run was taken.
        auto run_type = [&](int g_, int n_, Run& Rn) {
          const int end = g_ + n_;
          Grp T;
          int e = g_;
          while (true) {
            if (e + 1 < end) load_group(e + 1, T);
            compute(Rn.first, Rn.bq);
            if (++e >= end) break;
            if (e + 1 < end) load_group(e + 1, Rn.first);
            compute(T, Rn.bq);
            if (++e >= end) break;
          }
        };
        // Matrix rows of run r -> Rn.bq.  ALWAYS four loads: beyond the last run (`have` false) they read four cache
        // lines of type 0 that nobody uses - the number of vector-memory operations in flight behind any fetch is
        // then the same on every path, so the compiler can wait for a run's rows with a COUNTED s_waitcnt vmcnt(n)
        // and leave the younger fetches in flight (vmcnt retires in order; with conditional loads it must drain).
        auto fetch = [&](bool have, int r, int& g_, int& n_, Run& Rn, const float* tm) {
          const int rc = have ? r : 0;
          g_ = __builtin_amdgcn_readfirstlane(r_runs[rc]);
          n_ = __builtin_amdgcn_readfirstlane(r_runs[rc + 1]) - g_;
          const int type = have ? (__builtin_amdgcn_readfirstlane(grp_x[4 * g_]) & 0xff) : 0;
          const float* bp = tm + (size_t)type * kTMatFloats + (have ? boff : 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) Rn.bq[i] = ld4(bp + i * 128);
        };
        // dynamically assigned runs (beyond the two static ones per wave) come from an LDS counter: the runs differ in
        // length and in how long their matrix rows take to arrive (a static split left the slowest wave 20 % behind).
        auto next_run = [&]() {
          int r = 0;
          if (lane == 0) r = atomicAdd(run_ctr, 1);
          return __builtin_amdgcn_readfirstlane(r);
        };
        auto take = [&](int r, int& g_, int& n_, Run& Rn) {  // r < nrun
          fetch(true, r, g_, n_, Rn, tm_s);
          load_group(g_, Rn.first);
        };
        // `landed`: the rows are consumed here (an empty asm that reads and rewrites the registers), so the compiler
        // places its s_waitcnt vmcnt HERE.
        auto landed = [](f32x4 (&b)[4]) {
          asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : : "memory");
        };
        // the first two runs of a wave are fixed; the rest comes from the counter.  (Loads in program order on every
        // path: image, P, Q - so that the counted waits below hold.)
        if (kRunsEarly < 1) fetch_P(s);
        if (kRunsEarly < 2) fetch_Q(s);
        haveP = sP; gP = sgP; nP = snP;
        haveQ = sQ; gQ = sgQ; nQ = snQ;
        if (haveP) load_group(gP, P.first);
        if (haveQ) load_group(gQ, Q.first);
        // Runs are taken in the order P, Q, P, ... (run `wave + 16` exists only if run `wave` does).  Inside the loop
        // every path issues the same loads in the same order, so each `landed` is a counted wait that leaves the other
        // run's rows in flight; the first counter value beyond the last run leaves the loop through a tail that issues
        // no loads at all.
        if (haveP) {
          if (!haveQ) {
            landed(P.bq);
            run_type(gP, nP, P);
          } else {
            while (true) {
              landed(P.bq);
              run_type(gP, nP, P);
              const int rP = next_run();
              if (rP >= nrun) {
                landed(Q.bq);
                run_type(gQ, nQ, Q);
                break;
              }
              take(rP, gP, nP, P);
              landed(Q.bq);
              run_type(gQ, nQ, Q);
              const int rQ = next_run();
              if (rQ >= nrun) {
                landed(P.bq);
                run_type(gP, nP, P);
                break;
              }
              take(rQ, gQ, nQ, Q);
            }
          }
        }
        // A wave without a run P or Q leaves that run's four loads unused - and, to the compiler, in flight until the
        // registers are written again, which would be in the pool: its wait there would wait for fetch_step0's transfers
        // as well.  Landed here, in front of the mid-step barrier, the wait costs nothing.
        landed(P.bq);
        landed(Q.bq);
      }
      // this step's update image -> LDS (ordered by the mid-step barrier); step 0's is there already (fetch_step0)
      if (s > 0) {
#pragma unroll
        for (int i = 0; i < kNPf; ++i)
          if (4 * (tid + i * kThreads) < kUpdLds) st4(wupd + 4 * (tid + i * kThreads), pf[i]);
      }
      const bool mstamp = stamp && c == c_begin && s == 1;
      if (mstamp && lane == 0) stamp[16 + wave] = __builtin_amdgcn_s_memtime();
      // Mid-step barrier: every message is in LDS and every read of h by the message phase is done (h is updated in
      // place below); the update image of this step is in place too.
      lds_barrier();
      if (tid == 0) *run_ctr = 2 * kWaves;  // for the next step's message phase (ordered by the end-of-step barrier)
      if (mstamp && tid == 0) stamp[12] = __builtin_amdgcn_s_memtime();
      if (stamp && tid == 0 && c == c_begin && s == 1) t_msg = __builtin_amdgcn_s_memtime();

      atom_phase(std::false_type{}, s);
      // End-of-step barrier: every row of h is updated, every read of the message buffer and of the update image is
      // done.  (LDS traffic only: the run prefetch above stays in flight across it.)
      lds_barrier();
      if (stamp && c == c_begin && s < 2 && tid == 0) stamp[14 + s] = __builtin_amdgcn_s_memtime();
    }
    if (stamp && tid == 0) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      t_steps += t - t_mark;
      t_mark = t;
    }

    // the message buffer and the update image are idle from here to the next chunk's step 0: its inputs start their way
    // (the next record and descriptor, requested a whole chunk's steps ago, are landed by name first: with nothing it knows
    //  of in flight the compiler places no s_waitcnt of its own into the pool, which would wait for the transfers as well)
    asm volatile(""
                 : "+v"(rec_n8.x), "+v"(rec_n8.y), "+v"(rec_n4), "+v"(dsc_next.x), "+v"(dsc_next.y), "+v"(dsc_next.z),
                   "+v"(dsc_next.w)
                 :
                 : "memory");
    if (c + 1 < c_end) fetch_step0(dsc_next, c + 1);
    pool(M, m0, g);
    lds_barrier();  // the record / h buffers are rewritten by the next chunk's prologue
    if (two_rec) use_record(recl == recl0 ? recl0 + rec_lds : recl0);
    if (stamp && tid == 0) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      t_pool += t - t_mark;
      t_mark = t;
    }
  }
  if (stamp && tid == 0) {
    stamp[1] = t_pro;
    stamp[2] = t_steps;
    stamp[3] = t_pool;
    stamp[4] = (unsigned long long)(c_end - c_begin);
    stamp[5] = t_msg;
    stamp[7] = __builtin_amdgcn_s_memtime();
  }
}

}  // namespace
}  // namespace enc

bool encoder_typed_supported(int N, int E, int D, int S, int Vb) {
  using namespace enc;
  if (D != kD || S < 0) return false;
  // Any padded shape: what bounds a chunk is what a molecule HOLDS - kept rows <= 256, valid edges <= 512, in-degrees
  // <= 255 (640 valid edges for padded E > 512) - and that is checked per batch by the plan kernels
  // (PlanHeader::overflow), not here.
  if (N < 1 || N > 0xffff || E < 0 || E > 0xffff) return false;
  if (Vb < 1 || Vb > kTVbMax) return false;
  return true;
}

size_t encoder_typed_prepared_bytes(int S, int Vb, bool x3) {
  return enc::typed_prepared_floats(S, Vb, x3) * sizeof(float);
}

int launch_encoder_typed_prepare(const float* weights, const float* bond_table, int K, int S, int Vb, bool x3,
                                 void* prepared, hipStream_t s) {
  if (S <= 0) return IMPNN_OK;
  enc::TImageParams ip{};
  ip.weights = weights;
  ip.bond_table = bond_table;
  ip.prepared = static_cast<float*>(prepared);
  ip.K = K;
  ip.S = S;
  ip.Vb = Vb;
  ip.x3 = x3 ? 1 : 0;
  ip.step_floats = impnn_encoder_step_floats(enc::kD, K);
  return enc::launch_typed_image(ip, s);
}

// ---- the image with the step-0 message table behind it (encoder_layout.h: M0Header)
size_t encoder_typed_prepared_bytes_atoms(int S, int Va, int Vb, bool x3) {
  return (enc::typed_prepared_floats(S, Vb, x3) + enc::m0_table_floats(S, Va, Vb)) * sizeof(float);
}

int launch_encoder_typed_prepare_atoms(const float* weights, const float* bond_table, const float* atom_table, int Va,
                                       int K, int S, int Vb, bool x3, void* prepared, hipStream_t s) {
  using namespace enc;
  // the plain image first: its typed_image_kernel clears the header, so a shape beyond the cap ends here with "none"
  if (int rc = launch_encoder_typed_prepare(weights, bond_table, K, S, Vb, x3, prepared, s)) return rc;
  if (m0_table_floats(S, Va, Vb) == 0) return IMPNN_OK;
  float* img = static_cast<float*>(prepared);
  const size_t uslot = x3 ? kXUpdSlot : kTUpdSlot;
  const int waves = Vb * ((Va + 4) >> 2);
  typed_m0_kernel<<<(waves + 3) / 4, 256, 0, s>>>(img + (size_t)S * uslot, atom_table, img + typed_prepared_floats(S, Vb, x3),
                                                  reinterpret_cast<M0Header*>(img + (x3 ? kXUpdLds : kTUpdLds)), Va, Vb, S);
  return check_launch("typed_m0");
}

// ---- the same with the step-0 gate table behind the message table (encoder_layout.h: G0Header); where no message table
// is built there is no gate table either, and size and image are the with-atoms entry's
size_t encoder_typed_prepared_bytes_gates(int S, int Va, int Vb, bool x3) {
  return encoder_typed_prepared_bytes_atoms(S, Va, Vb, x3) + enc::g0_table_floats(S, Va, Vb) * sizeof(float);
}

int launch_encoder_typed_prepare_gates(const float* weights, const float* bond_table, const float* atom_table, int Va,
                                       int K, int S, int Vb, bool x3, void* prepared, hipStream_t s) {
  using namespace enc;
  if (int rc = launch_encoder_typed_prepare_atoms(weights, bond_table, atom_table, Va, K, S, Vb, x3, prepared, s)) return rc;
  if (g0_table_floats(S, Va, Vb) == 0) return IMPNN_OK;
  float* img = static_cast<float*>(prepared);
  float* g0 = img + typed_prepared_floats(S, Vb, x3) + m0_table_floats(S, Va, Vb);
  G0Header* hdr = reinterpret_cast<G0Header*>(img + (x3 ? kXUpdLds : kTUpdLds) + kG0HeaderFloatOff);
  const int tiles = (Va + 16) / 16;  // Va + 1 columns
  if (x3)
    typed_g0_kernel<true><<<tiles, 64, 0, s>>>(img, atom_table, g0, hdr, Va, Vb, S);
  else
    typed_g0_kernel<false><<<tiles, 64, 0, s>>>(img, atom_table, g0, hdr, Va, Vb, S);
  return check_launch("typed_g0");
}

int launch_encoder_typed_run(const EncoderArgs& a, const enc::Ws& w, hipStream_t s) {
  using namespace enc;
  char* base = static_cast<char*>(a.workspace);
  TEncParams ep{};
  const size_t S1 = a.S > 0 ? a.S : 1;
  const bool x3 = a.mode == 3;
  const size_t uslot = x3 ? kXUpdSlot : kTUpdSlot;
  for (int g = 0; g < a.n_ions; ++g) {
    const float* prep;
    if (a.prepared[g]) {
      if (!aligned16(a.prepared[g])) return fail(IMPNN_E_BADARG, "encoder_fused: prepared weights must be 16B aligned");
      prep = static_cast<const float*>(a.prepared[g]);
    } else {  // canonical weights: build the images into the workspace first
      float* img = reinterpret_cast<float*>(base + w.img_off) + (size_t)g * typed_prepared_floats(a.S, a.Vb, x3);
      if (int rc = launch_encoder_typed_prepare(a.weights[g], a.bond_table, a.K, a.S, a.Vb, x3, img, s)) return rc;
      prep = img;
    }
    ep.upd[g] = prep;
    ep.tmat[g] = prep + S1 * uslot;
    ep.m0[g] = prep + typed_prepared_floats(a.S, a.Vb, x3);
    ep.g0[g] = ep.m0[g] + m0_table_floats(a.S, a.Va, a.Vb);
    ep.pooled[g] = a.pooled[g];
  }
  ep.atom_table = a.atom_table;
  ep.nsub = reinterpret_cast<const int32_t*>(base + w.nsub_off);
  ep.desc = reinterpret_cast<const int32_t*>(base + w.desc_off);
  ep.rec = reinterpret_cast<const unsigned char*>(base + w.rec_off);
  ep.slist = reinterpret_cast<const uint32_t*>(base + w.slist_off);
  ep.header = reinterpret_cast<const PlanHeader*>(base);
  ep.n_ions = a.n_ions; ep.B = a.B; ep.S = a.S; ep.Va = a.Va; ep.Vb = a.Vb; ep.max_sub = w.max_sub;
  ep.ln_eps = a.ln_eps;
  ep.stamps = nullptr;
  {
    size_t sb = 0;
    void* sp = debug_stamp_buffer(&sb);
    if (sp && sb >= (size_t)w.nwg * 32 * sizeof(unsigned long long)) ep.stamps = static_cast<unsigned long long*>(sp);
  }
  ep.upd_slot = (int)uslot;
  ep.ecap = tecap_of(a.E);
  ep.rec_lds = trec_lds_bytes(a.Vb, ep.ecap);
  const bool big3 = x3 && ep.ecap == kTECapBig;  // mode 3 on 640-edge chunks: unpadded h rows (kTHSBig3)
  void (*kern)(TEncParams) =
      big3 ? (ep.stamps ? encoder_typed_kernel<true, true, kTHSBig3> : encoder_typed_kernel<false, true, kTHSBig3>)
      : x3 ? (ep.stamps ? encoder_typed_kernel<true, true> : encoder_typed_kernel<false, true>)
           : (ep.stamps ? encoder_typed_kernel<true, false> : encoder_typed_kernel<false, false>);
  if (int rc = ensure_lds_limit((const void*)kern, big3 ? (ep.stamps ? 10 : 9) : (ep.stamps ? 5 : 4) + (x3 ? 2 : 0))) return rc;
  size_t lds = lds_fixed_bytes(x3, a.Vb, ep.ecap, big3 ? kTHSBig3 : kTHS);
  const size_t atab_bytes = ((size_t)a.Va + 1) * kTAS * sizeof(float);
  ep.atab_lds = lds + atab_bytes <= 160 * 1024;
  if (ep.atab_lds) lds += atab_bytes;
  profile_record_start(s);
  kern<<<w.nwg, kThreads, lds, s>>>(ep);
  profile_record_stop(s);
  return check_launch("encoder_typed");
}

}  // namespace impnn
