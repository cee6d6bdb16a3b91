// The GatedUpdate of the wide encoder in mode f32x3 (encoder_wide.hip has the stage list): wide_update_x3 on 64-row
// tiles and wide_update_x3b on 128-row tiles, both bf16x9.
#include "wide_device.h"

namespace impnn {
namespace wide {

// ------------------------------------------------------------------------------------------------------------
// a7 in mode IMPNN_ENCODER_F32X3_TYPED ("f32 (bf16x9 emulation)"): the same GatedUpdate with its three GEMMs on the bf16
// matrix pipe.  Every f32 operand is carried EXACTLY as three bf16 terms (x = b0 + b1 + b2: bf16 keeps fp32's exponent,
// 3 x 8 significant bits) and all nine cross products are accumulated in f32 - the f32 products themselves, summed in
// another order (encoder_typed.hip has the D = 32 form and the discussion of non-finite operands).  Nine
// v_mfma_f32_16x16x32_bf16 (16 cycles, 32 k) replace eight v_mfma_f32_16x16x4_f32 (32 cycles, 4 k): 9/16 of the matrix
// time, on a pipe that - unlike the exact-f32 one - co-executes with the vector ALU.
//   * the gate kernels arrive pre-split from the prepared image (wide_gu_image_x3_kernel), in 32-k slices of MFMA
//     B-operand order [plane][k octet][column][8 k]: a slice is copied global -> registers -> LDS verbatim;
//   * the rows ([h | agg], then [r*h | agg]) are split when a slice is parked in LDS (A-operand order
//     [plane][k octet][row][8 k]; 5.5 vector instructions per value);
//   * one workgroup of 8 waves per CU (a 32-k slice of [Wz|Wr] is 48 KB in three planes: two stages fill the LDS),
//     wave = 32 rows x NL feature tiles of z and of r: 72 MFMAs per wave and slice between barriers.
// ------------------------------------------------------------------------------------------------------------
constexpr int kGuX3Threads = 512;
// LDS bytes: two stages of (rows 12 KB + [Wz|Wr] slice 3 x 4 x 2D x 16 B) - phase 2 re-cuts the same memory into two
// stages of (rows + Wh slice) and the f32 copy of r*h - plus the LayerNorm partials
constexpr size_t gu_x3_lds_bytes(int D) { return 2 * (size_t)(12288 + 12 * 2 * D * 16) + 8 * kRT * 4; }

template <int NT>
__global__ __launch_bounds__(kGuX3Threads, 2) void wide_update_x3_kernel(GuParams p) {
  constexpr int D = 16 * NT, R = kRT, LDR = D + 4;
  constexpr int RG = 2, FG = 4, NL = NT / FG;
  constexpr int NS = NT;                     // 32-k slices of a 2D-deep GEMM
  constexpr int UA = 3 * 4 * R;              // 16-byte units of a row slice (768)
  constexpr int UB1 = 3 * 4 * 2 * D;         // ... of a [Wz|Wr] slice
  constexpr int UB2 = 3 * 4 * D;             // ... of a Wh slice
  constexpr int ST1 = UA + UB1, ST2 = UA + UB2;  // stage sizes (units)
  constexpr int kQ1 = (UB1 + kGuX3Threads - 1) / kGuX3Threads, kQ2 = (UB2 + kGuX3Threads - 1) / kGuX3Threads;
  static_assert(NL >= 1 && NT % 2 == 0, "tile shape");
  static_assert((size_t)2 * ST2 * 16 + (size_t)R * LDR * 4 <= (size_t)2 * ST1 * 16, "phase 2 fits phase 1's stages");
  extern __shared__ __align__(16) unsigned char smem_b[];
  uint4* const stage = reinterpret_cast<uint4*>(smem_b);                       // phase 1: 2 x ST1 units
  float* const rhs = reinterpret_cast<float*>(smem_b + (size_t)2 * ST2 * 16);  // phase 2: R x LDR f32, r * h
  float* const part = reinterpret_cast<float*>(smem_b + (size_t)2 * ST1 * 16);  // 2 x FG x R LayerNorm partials
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, a = lane & 15, q = lane >> 4;
  const int rg = wv % RG, fg = wv / RG;
  const int64_t row0 = (int64_t)blockIdx.x * p.tile_rows;
  const int end = p.meta[kMetaEnd];
  if (row0 >= end) return;
  const int g = (p.n_ions > 1 && row0 >= p.meta[kMetaBase + 1]) ? 1 : 0;
  const int64_t ion_end = p.meta[kMetaBase + g] + p.meta[kMetaRows + g];
  const int64_t row_end = row0 + p.tile_rows < ion_end ? row0 + p.tile_rows : ion_end;
  if (row0 >= row_end) return;
  const float* img = p.img[g] + p.gu_off;
  const uint4* P1 = reinterpret_cast<const uint4*>(img);
  const uint4* P2 = P1 + (size_t)NS * UB1;
  const float* bias = reinterpret_cast<const float*>(P2 + (size_t)NS * UB2);  // bz br bh gamma beta
  // a thread's piece of a row slice: row a_row, k = 4 a_pc .. 4 a_pc + 3 of the slice's 32
  const int a_row = tid >> 3, a_pc = tid & 7;
  const float* hsrc = p.h + (row0 + a_row) * D + 4 * a_pc;
  // the row's aggregated messages: two sources (wide_iota_kernel), as float offsets from p.agg
  const int goff0 = agg_off(p.c2a[row0 + a_row], p.m_off, D) + 4 * a_pc, goff1 = agg_off(p.c2b[row0 + a_row], p.m_off, D) + 4 * a_pc;
  // unit (plane, k octet a_pc >> 1, row a_row), 8-byte half a_pc & 1
  const int a_unit = (a_pc >> 1) * R + a_row, a_half = a_pc & 1;
  auto park_rows = [&](uint4* st, f32x4_t v) {  // 4 values -> three planes of 4 bf16
    unsigned w0[2], w1[2], w2[2];
    split_pair(v[0], v[1], w0[0], w1[0], w2[0]);
    split_pair(v[2], v[3], w0[1], w1[1], w2[1]);
    uint2* s2 = reinterpret_cast<uint2*>(st);
    s2[(0 * 4 * R + a_unit) * 2 + a_half] = make_uint2(w0[0], w0[1]);
    s2[(1 * 4 * R + a_unit) * 2 + a_half] = make_uint2(w1[0], w1[1]);
    s2[(2 * 4 * R + a_unit) * 2 + a_half] = make_uint2(w2[0], w2[1]);
  };
  struct Pre {
    f32x4_t av;
    uint4 bv[kQ1];
  };
  Pre preA, preB;
  auto fetch1 = [&](int u, Pre& pre) {
#pragma unroll
    for (int i = 0; i < kQ1; ++i)
      if (tid + kGuX3Threads * i < UB1) pre.bv[i] = P1[(size_t)u * UB1 + tid + kGuX3Threads * i];
    // (a slice of aggregated messages: the row's two sources, first slot first - the Reduce's order)
    pre.av = u < NS / 2 ? ldv4(hsrc + 32 * u) : ldv4(p.agg + goff0 + 32 * (u - NS / 2)) + ldv4(p.agg + goff1 + 32 * (u - NS / 2));
  };
  auto park1 = [&](uint4* st, const Pre& pre) {
#pragma unroll
    for (int i = 0; i < kQ1; ++i)
      if (tid + kGuX3Threads * i < UB1) st[UA + tid + kGuX3Threads * i] = pre.bv[i];
    park_rows(st, pre.av);
  };
  f32x4_t z[2][NL], rr[2][NL];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const int f = 16 * (fg * NL + TL) + a;
    const float b0 = bias[f], b1 = bias[D + f];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      z[rt][TL] = f32x4_t{b0, b0, b0, b0};
      rr[rt][TL] = f32x4_t{b1, b1, b1, b1};
    }
  }
  // operands of one slice: rows (A) and kernel columns (B), three planes each
  auto read_a = [&](const uint4* st, int rt, bf16x8_t (&av)[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      av[pl] = __builtin_bit_cast(bf16x8_t, st[(pl * 4 + q) * R + 32 * rg + 16 * rt + a]);
  };
  auto read_b = [&](const uint4* st, int ncols, int col, bf16x8_t (&bv)[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) bv[pl] = __builtin_bit_cast(bf16x8_t, st[UA + (pl * 4 + q) * ncols + col]);
  };
  // acc += A B: all nine cross products, smallest first
  auto mma9 = [&](f32x4_t& acc, const bf16x8_t (&av)[3], const bf16x8_t (&bv)[3]) {
    acc = mfma_bf16(av[2], bv[2], acc);
    acc = mfma_bf16(av[1], bv[2], acc);
    acc = mfma_bf16(av[2], bv[1], acc);
    acc = mfma_bf16(av[0], bv[2], acc);
    acc = mfma_bf16(av[2], bv[0], acc);
    acc = mfma_bf16(av[1], bv[1], acc);
    acc = mfma_bf16(av[0], bv[1], acc);
    acc = mfma_bf16(av[1], bv[0], acc);
    acc = mfma_bf16(av[0], bv[0], acc);
  };
  // One slice of phase 1 on stage `cur` while slice u + 1 is parked in stage `oth`.  The MFMAs of a wave are paced by
  // the matrix pipe (16 cycles each); everything else of the iteration - the LDS reads of the second feature tile's
  // operands, the split of the next row slice and its LDS stores - is interleaved with them (sched_group_barrier:
  // without it the compiler emits reads, stores and MFMAs as three serial blocks and the pipe idles half the time).
  // (Row tiles beyond tile_rows are multiplied too - wasted only in launches too small to fill the chip - so that
  //  the iteration is one basic block.)
  auto slice1 = [&](const uint4* cur, uint4* oth, const Pre* pre, bool do_park) {
    bf16x8_t av[2][3], bz[NL][3], br[NL][3];
    read_a(cur, 0, av[0]);
    read_a(cur, 1, av[1]);
    read_b(cur, 2 * D, 16 * (fg * NL) + a, bz[0]);
    read_b(cur, 2 * D, D + 16 * (fg * NL) + a, br[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int TL = 1; TL < NL; ++TL) {
      read_b(cur, 2 * D, 16 * (fg * NL + TL) + a, bz[TL]);
      read_b(cur, 2 * D, D + 16 * (fg * NL + TL) + a, br[TL]);
    }
    if (do_park) park1(oth, *pre);
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      mma9(z[0][TL], av[0], bz[TL]);
      mma9(z[1][TL], av[1], bz[TL]);
      mma9(rr[0][TL], av[0], br[TL]);
      mma9(rr[1][TL], av[1], br[TL]);
    }
    // 36 NL MFMAs; 6 (NL - 1) LDS reads, ~10 LDS stores and ~45 vector instructions to hide between them
#pragma unroll
    for (int i = 0; i < 6 * (NL - 1); ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // VALU
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
    }
  };
  fetch1(0, preA);
  fetch1(1, preB);
  park1(stage, preA);
  __syncthreads();
  float hreg[2][NL][4];
  auto load_hreg = [&]() {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int TL = 0; TL < NL; ++TL)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          hreg[rt][TL][gq] = p.h[(row0 + 32 * rg + 16 * rt + 4 * q + gq) * D + 16 * (fg * NL + TL) + a];
  };
  // iteration u: slice u is in stage u & 1, slice u + 1 in registers, slice u + 2 is requested
  for (int u = 0; u < NS; u += 2) {
    if (u + 2 < NS) fetch1(u + 2, preA);
    else load_hreg();
    slice1(stage, stage + ST1, &preB, true);
    __syncthreads();
    if (u + 3 < NS) fetch1(u + 3, preB);
    slice1(stage + ST1, stage, &preA, u + 2 < NS);
    __syncthreads();
  }
  // ---- gates; r * h (f32) into LDS: phase 2 parks its first NS / 2 row slices from there
  struct Pre2 {
    f32x4_t av;
    uint4 bv[kQ2];
  };
  Pre2 qA, qB;
  auto fetch2 = [&](int u, Pre2& pre) {
#pragma unroll
    for (int i = 0; i < kQ2; ++i)
      if (tid + kGuX3Threads * i < UB2) pre.bv[i] = P2[(size_t)u * UB2 + tid + kGuX3Threads * i];
    if (u >= NS / 2) pre.av = ldv4(p.agg + goff0 + 32 * (u - NS / 2)) + ldv4(p.agg + goff1 + 32 * (u - NS / 2));
  };
  auto park2 = [&](int u, uint4* st, const Pre2& pre) {
#pragma unroll
    for (int i = 0; i < kQ2; ++i)
      if (tid + kGuX3Threads * i < UB2) st[UA + tid + kGuX3Threads * i] = pre.bv[i];
    park_rows(st, u < NS / 2 ? ldv4(rhs + a_row * LDR + 32 * u + 4 * a_pc) : pre.av);
  };
  fetch2(0, qA);
  fetch2(1, qB);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        z[rt][TL][gq] = fsig(z[rt][TL][gq]);
        rhs[(32 * rg + 16 * rt + 4 * q + gq) * LDR + 16 * (fg * NL + TL) + a] = gu_rh(rr[rt][TL][gq], hreg[rt][TL][gq]);
      }
  f32x4_t tt[2][NL];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const float b2 = bias[2 * D + 16 * (fg * NL + TL) + a];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) tt[rt][TL] = f32x4_t{b2, b2, b2, b2};
  }
  __syncthreads();  // r * h complete (and every read of phase 1's stages is done)
  uint4* const stage2 = stage;  // 2 x ST2 units
  park2(0, stage2, qA);
  __syncthreads();
  auto slice2 = [&](const uint4* cur, int u_next, uint4* oth, const Pre2* pre, bool do_park) {
    bf16x8_t av[2][3], bv[NL][3];
    read_a(cur, 0, av[0]);
    read_a(cur, 1, av[1]);
    read_b(cur, D, 16 * (fg * NL) + a, bv[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int TL = 1; TL < NL; ++TL) read_b(cur, D, 16 * (fg * NL + TL) + a, bv[TL]);
    if (do_park) park2(u_next, oth, *pre);
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      mma9(tt[0][TL], av[0], bv[TL]);
      mma9(tt[1][TL], av[1], bv[TL]);
    }
#pragma unroll
    for (int i = 0; i < 3 * (NL - 1); ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
    }
  };
  for (int u = 0; u < NS; u += 2) {
    if (u + 2 < NS) fetch2(u + 2, qA);
    slice2(stage2, u + 1, stage2 + ST2, &qB, true);
    __syncthreads();
    if (u + 3 < NS) fetch2(u + 3, qB);
    slice2(stage2 + ST2, u + 2, stage2, &qA, u + 2 < NS);
    __syncthreads();
  }
  // ---- blend, LayerNorm over the D features of a row, residual (models/layers.py:150-156): as wide_update_kernel
  float sum[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float sacc = 0.f;
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const float hv = hreg[rt][TL][gq];
        const float nv = gu_blend(z[rt][TL][gq], hv, tt[rt][TL][gq]);
        tt[rt][TL][gq] = nv;
        sacc += nv;
      }
      sum[rt][gq] = row16_sum_f(sacc);
      if (a == 0) part[fg * R + 32 * rg + 16 * rt + 4 * q + gq] = sum[rt][gq];
    }
  __syncthreads();
  float mean[2][4], inv[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int rl = 32 * rg + 16 * rt + 4 * q + gq;
      float ms = 0.f;
#pragma unroll
      for (int f2 = 0; f2 < FG; ++f2) ms += part[f2 * R + rl];
      mean[rt][gq] = ms * (1.0f / D);
      float vs = 0.f;
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const float dv = tt[rt][TL][gq] - mean[rt][gq];
        vs = fmaf(dv, dv, vs);
      }
      vs = row16_sum_f(vs);
      if (a == 0) part[FG * R + fg * R + rl] = vs;
    }
  __syncthreads();
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int rl = FG * R + 32 * rg + 16 * rt + 4 * q + gq;
      float vs = 0.f;
#pragma unroll
      for (int f2 = 0; f2 < FG; ++f2) vs += part[f2 * R + rl];
      inv[rt][gq] = gu_inv_std(vs, 1.0f / D, p.eps);
    }
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const int f = 16 * (fg * NL + TL) + a;
    const float gm = bias[3 * D + f], bt = bias[4 * D + f];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int64_t row = row0 + 32 * rg + 16 * rt + 4 * q + gq;
        if (row < row_end)
          p.h[row * D + f] = gu_out(tt[rt][TL][gq], mean[rt][gq], inv[rt][gq], gm, bt, hreg[rt][TL][gq]);
      }
  }
}

// ------------------------------------------------------------------------------------------------------------
// The same update on 128-row tiles (batches that fill the chip): per 32-k slice the 48 KB of pre-split gate kernels are
// shared by twice the rows, and a wave multiplies 64 rows x NL feature tiles of z and of r - 144 MFMAs per slice for 24
// operand fetches (the 64-row form: 72 for 18), so the LDS traffic per MFMA is 0.67 of the 64-row kernel's and the L2 -> LDS
// traffic of the kernels half.  One workgroup of 8 waves per CU, 256 VGPRs per lane.
//   * kernel slices go global -> LDS directly (global_load_lds_dwordx4: 16 B per lane, a wave's 64 lanes fill 1 KB of
//     consecutive LDS; no staging registers, no LDS store instructions); slice u + 1 lands in the other stage while
//     slice u is multiplied;
//   * row slices go global -> registers (one slice ahead) -> split -> the other stage, at the top of a slice;
//   * the nine products of an output tile form a dependent chain: the MFMAs are issued product by product ACROSS the
//     wave's four chains of a row tile (a chain's next link is four instructions away), and the operands of the next
//     row tile are requested in front of them;
//   * the split of slice u + 1's rows and their LDS stores sit between the MFMAs of slice u's first row tile
//     (sched_group_barrier): the bf16 pipe co-executes with the vector ALU;
//   * phase 2 re-cuts the LDS into two (rows + Wh slice) stages and an unpadded f32 copy of r * h - 160 KB at D = 128 -
//     and runs like phase 1 (one barrier per slice); the LayerNorm partials reuse a stage at the end;
//   * the tiles of the last, partial round are cut into 16-row pieces (wide_update_x3b_kernel below, MINI).
// ------------------------------------------------------------------------------------------------------------
// LDS: phase 1 two stages of (rows 24 KB + [Wz|Wr] slice); phase 2 re-cuts the same memory into two row stages, two Wh
// stages and the f32 copy of r * h (unpadded) - 160 KB at D = 128; the LayerNorm partials reuse the stages at the end
constexpr size_t gu_x3b_lds_bytes(int D) {
  const size_t p1 = 2 * (size_t)(3 * 4 * kRT3 * 16 + 12 * 2 * D * 16);
  const size_t p2 = 2 * (size_t)(3 * 4 * kRT3 * 16 + 12 * D * 16) + (size_t)kRT3 * D * 4;
  return p1 > p2 ? p1 : p2;
}


template <int NT, bool MINI>
__device__ __forceinline__ void x3b_tile(const GuParams& p, const int64_t row0, const int g, unsigned char* smem_b) {
  constexpr int D = 16 * NT, R = kRT3, LDR = D, T = kGuX3Threads;
  constexpr int RG = 2, FG = 4, NL = NT / FG, RTW = R / (16 * RG);  // a wave: RTW = 4 row tiles x NL feature tiles
  constexpr int NS = NT;                     // 32-k slices of a 2D-deep GEMM
  constexpr int UA = 3 * 4 * R;              // 16-byte units of a row slice
  constexpr int UB1 = 3 * 4 * 2 * D;         // ... of a [Wz|Wr] slice
  constexpr int UB2 = 3 * 4 * D;             // ... of a Wh slice
  constexpr int ST1 = UA + UB1;
  constexpr int RP = R / 64;                 // row pieces a thread parks per slice
  static_assert(NL >= 1 && NT % 2 == 0 && NS >= 4 && RTW == 4 && RP == 2, "tile shape");
  static_assert(UB1 % 64 == 0 && UB2 % 64 == 0, "a kernel slice is whole 1 KB wave transfers");
  constexpr int ST2 = UA + UB2;
  static_assert((size_t)2 * ST2 * 16 + (size_t)R * LDR * 4 <= 160 * 1024, "phase 2 fits the LDS");
  static_assert((size_t)8 * R * 4 <= (size_t)2 * ST2 * 16, "the LayerNorm partials fit the stages");
  uint4* const stage = reinterpret_cast<uint4*>(smem_b);                                  // phase 1: 2 x ST1 units
  uint4* const stage2 = stage;                                                            // phase 2: 2 x ST2 units (rows | Wh slice)
  float* const rhs = reinterpret_cast<float*>(smem_b + (size_t)2 * ST2 * 16);             // phase 2: R x LDR f32, r * h
  float* const part = reinterpret_cast<float*>(smem_b);                                   // epilogue: 2 x FG x R LayerNorm partials
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, a = lane & 15, q = lane >> 4;
  const int rg = wv % RG, fg = wv / RG;
  // MINI: a 16-row piece of a tile of the last, partial round (wide_update_x3b_kernel): the same stages and slices, but
  // only the waves of row group 0 multiply, and only their first row tile
  auto active = [&](int rt) { return !MINI || (rg == 0 && rt == 0); };  // (wave-uniform)
  WIDE_STAMP(p.stamps, 0);
  WIDE_STAMP_REAL(p.stamps, 5);
  const float* img = p.img[g] + p.gu_off;
  const uint4* P1 = reinterpret_cast<const uint4*>(img);
  const uint4* P2 = P1 + (size_t)NS * UB1;
  const float* bias = reinterpret_cast<const float*>(P2 + (size_t)NS * UB2);  // bz br bh gamma beta
  // a thread's pieces of a row slice: rows a_row and a_row + 64, k = 4 a_pc .. 4 a_pc + 3 of the slice's 32
  const int a_row = tid >> 3, a_pc = tid & 7;
  const float* hsrc = p.h + (row0 + a_row) * D + 4 * a_pc;
  // the aggregated messages of the thread's two rows: two sources each (wide_iota_kernel), as float offsets from p.agg
  int goff[RP][2];
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const int ca = p.c2a[row0 + a_row + 64 * i], cb = p.c2b[row0 + a_row + 64 * i];
    goff[i][0] = agg_off(ca, p.m_off, D) + 4 * a_pc;
    goff[i][1] = agg_off(cb, p.m_off, D) + 4 * a_pc;
  }
  f32x4_t pavb[RP];  // the second source's piece (added when the slice is parked)
  const int a_unit = (a_pc >> 1) * R + a_row, a_half = a_pc & 1;  // unit (plane, k octet a_pc >> 1, row), 8-byte half
  auto park_rows = [&](uint4* st, f32x4_t v, int piece) {  // 4 values -> three planes of 4 bf16
    unsigned w0[2], w1[2], w2[2];
    split_pair(v[0], v[1], w0[0], w1[0], w2[0]);
    split_pair(v[2], v[3], w0[1], w1[1], w2[1]);
    uint2* s2 = reinterpret_cast<uint2*>(st);
    const int un = a_unit + 64 * piece;
    s2[(0 * 4 * R + un) * 2 + a_half] = make_uint2(w0[0], w0[1]);
    s2[(1 * 4 * R + un) * 2 + a_half] = make_uint2(w1[0], w1[1]);
    s2[(2 * 4 * R + un) * 2 + a_half] = make_uint2(w2[0], w2[1]);
  };
  // `units` 16-byte units from global to LDS, verbatim: wave w moves units 64 (8 i + w) .. + 63 with its i-th instruction
  auto dma = [&](const uint4* src, uint4* dst, int units) {
#pragma unroll
    for (int i = 0; i < (units + T - 1) / T; ++i) {
      const int ub = 64 * (8 * i + wv);
      if (ub < units)  // (wave-uniform)
        __builtin_amdgcn_global_load_lds((const void*)(src + ub + lane), (lds_ptr_t)(dst + ub), 16, 0, 0);
    }
  };
  // workgroup barrier behind everything this wave has in flight (kernel slices on their way into LDS included)
  auto wg_barrier = [&]() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  f32x4_t pav[RP];
  auto fetch_rows1 = [&](int u) {
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      if (u < NS / 2) {
        pav[i] = ldv4(hsrc + 32 * u + (size_t)64 * i * D);
      } else {
        pav[i] = ldv4(p.agg + goff[i][0] + 32 * (u - NS / 2));
        pavb[i] = ldv4(p.agg + goff[i][1] + 32 * (u - NS / 2));
      }
    }
  };
  f32x4_t z[RTW][NL], rr[RTW][NL];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const int f = 16 * (fg * NL + TL) + a;
    const float b0 = bias[f], b1 = bias[D + f];
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt) {
      z[rt][TL] = f32x4_t{b0, b0, b0, b0};
      rr[rt][TL] = f32x4_t{b1, b1, b1, b1};
    }
  }
  auto read_a = [&](const uint4* st, int rt, bf16x8_t (&av)[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      av[pl] = __builtin_bit_cast(bf16x8_t, st[(pl * 4 + q) * R + 64 * rg + 16 * rt + a]);
  };
  float hreg[RTW][NL][4];
  auto load_hreg = [&]() {
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt)
      if (active(rt)) {
#pragma unroll
        for (int TL = 0; TL < NL; ++TL)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            hreg[rt][TL][gq] = p.h[(row0 + 64 * rg + 16 * rt + 4 * q + gq) * D + 16 * (fg * NL + TL) + a];
      }
  };
  // the nine products, smallest first: (row plane, kernel plane)
  constexpr int kPa[9] = {2, 1, 2, 0, 2, 1, 0, 1, 0}, kPb[9] = {2, 2, 1, 2, 0, 1, 1, 0, 0};
  auto slice1 = [&](const uint4* cur, uint4* oth, int u) {
    bf16x8_t bz[NL][3], br[NL][3], av[2][3];
    // operands in the order the products take them (plane 2 of both first): the first MFMA waits for 5 fetches, not 15
#pragma unroll
    for (int pl = 2; pl >= 0; --pl) {
      av[0][pl] = __builtin_bit_cast(bf16x8_t, cur[(pl * 4 + q) * R + 64 * rg + a]);
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        bz[TL][pl] = __builtin_bit_cast(bf16x8_t, cur[UA + (pl * 4 + q) * 2 * D + 16 * (fg * NL + TL) + a]);
        br[TL][pl] = __builtin_bit_cast(bf16x8_t, cur[UA + (pl * 4 + q) * 2 * D + D + 16 * (fg * NL + TL) + a]);
      }
    }
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt) {
      if (rt + 1 < RTW) read_a(cur, rt + 1, av[(rt + 1) & 1]);
      if (rt > 0) __builtin_amdgcn_sched_barrier(0);
      // Row tile 0 shares its scheduling region with the split of slice u + 1's rows (in the staging registers since the
      // last slice) and their LDS stores: vector instructions issue between the MFMAs of the bf16 pipe for free.
      if (rt == 0 && u + 1 < NS) {
        // (the slices of the aggregated messages: the row's two sources are added here - first slot first)
        park_rows(oth, u + 1 >= NS / 2 ? pav[0] + pavb[0] : pav[0], 0);
        if (!MINI) park_rows(oth, u + 1 >= NS / 2 ? pav[1] + pavb[1] : pav[1], 1);
      }
      if (active(rt)) {
#pragma unroll
        for (int pr = 0; pr < 9; ++pr)
#pragma unroll
          for (int TL = 0; TL < NL; ++TL) {
            z[rt][TL] = mfma_bf16(av[rt & 1][kPa[pr]], bz[TL][kPb[pr]], z[rt][TL]);
            rr[rt][TL] = mfma_bf16(av[rt & 1][kPa[pr]], br[TL][kPb[pr]], rr[rt][TL]);
          }
      }
      if (!MINI && rt == 0 && u + 1 < NS) {
#pragma unroll
        for (int i = 0; i < 6 * NL; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // VALU
        }
#pragma unroll
        for (int i = 0; i < 3 * NL; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (rt == 0) {
        if (u + 1 < NS) {  // slice u + 2's rows requested; slice u + 1's kernels on their way into the other stage
          if (u + 2 < NS) fetch_rows1(u + 2);  // (behind the LDS stores: a store behind a transfer in flight waits for it)
          dma(P1 + (size_t)(u + 1) * UB1, oth + UA, UB1);
        } else {
          load_hreg();
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  fetch_rows1(0);
  park_rows(stage, pav[0], 0);
  if (!MINI) park_rows(stage, pav[1], 1);
  __builtin_amdgcn_sched_barrier(0);
  fetch_rows1(1);
  dma(P1, stage + UA, UB1);
  wg_barrier();
  WIDE_STAMP(p.stamps, 1);
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    slice1(stage + (u & 1) * ST1, stage + ((u + 1) & 1) * ST1, u);
    wg_barrier();
  }
  WIDE_STAMP(p.stamps, 2);
  // ---- gates; r * h (f32) into LDS: phase 2 parks its first NS / 2 row slices from there
  auto fetch_rows2 = [&](int u) {    // (u >= NS / 2: the aggregated messages)
#pragma unroll
    for (int i = 0; i < RP; ++i) {
      pav[i] = ldv4(p.agg + goff[i][0] + 32 * (u - NS / 2));
      pavb[i] = ldv4(p.agg + goff[i][1] + 32 * (u - NS / 2));
    }
  };
  auto park2 = [&](uint4* st, int u) {
#pragma unroll
    for (int i = 0; i < (MINI ? 1 : RP); ++i)
      park_rows(st, u < NS / 2 ? ldv4(rhs + (a_row + 64 * i) * LDR + 32 * u + 4 * a_pc) : pav[i] + pavb[i], i);
  };
  // (every wave is past the last barrier of phase 1: the stages are free)
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt)) {
#pragma unroll
      for (int TL = 0; TL < NL; ++TL)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          if (MINI) z[rt][TL][gq] = fsig(z[rt][TL][gq]);  // (whole tiles: between the MFMAs of phase 2, slice2)
          rhs[(64 * rg + 16 * rt + 4 * q + gq) * LDR + 16 * (fg * NL + TL) + a] = gu_rh(rr[rt][TL][gq], hreg[rt][TL][gq]);
        }
    }
  f32x4_t tt[RTW][NL];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const float b2 = bias[2 * D + 16 * (fg * NL + TL) + a];
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt) tt[rt][TL] = f32x4_t{b2, b2, b2, b2};
  }
  __builtin_amdgcn_sched_barrier(0);
  dma(P2, stage2 + UA, UB2);  // (behind the LDS stores above: a store behind a transfer in flight would wait for it)
  wg_barrier();  // r * h complete
  park2(stage2, 0);
  wg_barrier();
  auto slice2 = [&](const uint4* cur, uint4* oth, int u) {
    bf16x8_t bv[NL][3], av[2][2][3];
#pragma unroll
    for (int pl = 2; pl >= 0; --pl) {  // (in the order the products take them)
      av[0][0][pl] = __builtin_bit_cast(bf16x8_t, cur[(pl * 4 + q) * R + 64 * rg + a]);
      av[0][1][pl] = __builtin_bit_cast(bf16x8_t, cur[(pl * 4 + q) * R + 64 * rg + 16 + a]);
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) bv[TL][pl] = __builtin_bit_cast(bf16x8_t, cur[UA + (pl * 4 + q) * D + 16 * (fg * NL + TL) + a]);
    }
#pragma unroll
    for (int rp = 0; rp < RTW / 2; ++rp) {  // two row tiles at a time: four chains
      if (rp + 1 < RTW / 2) {
        read_a(cur, 2 * rp + 2, av[(rp + 1) & 1][0]);
        read_a(cur, 2 * rp + 3, av[(rp + 1) & 1][1]);
      }
      if (rp > 0) __builtin_amdgcn_sched_barrier(0);
      if (rp == 0 && u + 1 < NS) park2(oth, u + 1);  // (between the MFMAs, as in phase 1)
      // the update gate's sigmoids are not needed before the blend: they ride between the MFMAs of the second row-tile
      // pair of slices 0 and 1 (two row tiles each) instead of standing in front of phase 2
      if (!MINI && rp == 1 && u < 2) {
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
          for (int TL = 0; TL < NL; ++TL)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) z[2 * u + r2][TL][gq] = fsig(z[2 * u + r2][TL][gq]);
      }
      if (active(2 * rp)) {  // (MINI: row tile 1 rides along with row tile 0 - its rows are never stored)
#pragma unroll
        for (int pr = 0; pr < 9; ++pr)
#pragma unroll
          for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
            for (int TL = 0; TL < NL; ++TL)
              tt[2 * rp + r2][TL] = mfma_bf16(av[rp & 1][r2][kPa[pr]], bv[TL][kPb[pr]], tt[2 * rp + r2][TL]);
      }
      if (!MINI && rp == 0 && u + 1 < NS) {
#pragma unroll
        for (int i = 0; i < 6 * NL; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        }
#pragma unroll
        for (int i = 0; i < 3 * NL; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        }
      }
      if (!MINI && rp == 1 && u < 2) {
#pragma unroll
        for (int i = 0; i < 9 * NL; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // VALU (two of every four are quarter-rate)
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (rp == 0 && u + 1 < NS) {
        if (u + 2 < NS && u + 2 >= NS / 2) fetch_rows2(u + 2);
        dma(P2 + (size_t)(u + 1) * UB2, oth + UA, UB2);  // slice u + 1's Wh slice straight from global
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // (the first slice of aggregated messages, NS / 2, is requested inside slice NS / 2 - 2 and parked inside NS / 2 - 1)
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    slice2(stage2 + (u & 1) * ST2, stage2 + ((u + 1) & 1) * ST2, u);
    wg_barrier();
  }
  WIDE_STAMP(p.stamps, 3);
  // ---- blend, LayerNorm over the D features of a row, residual (models/layers.py:150-156): as wide_update_kernel
  // sum over the 16 lanes of a quarter wave, all of the wave's rows step by step (a row's next step is 16 instructions
  // behind its last: no stall between dependent DPP operations)
  auto row16_sum_all = [&](float (&v)[RTW][4]) {
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int rt = 0; rt < RTW; ++rt)
        if (active(rt))
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            const int iv = __builtin_bit_cast(int, v[rt][gq]);
            const int o = st == 0 ? __builtin_amdgcn_update_dpp(0, iv, 0x121, 0xf, 0xf, true)
                          : st == 1 ? __builtin_amdgcn_update_dpp(0, iv, 0x122, 0xf, 0xf, true)
                          : st == 2 ? __builtin_amdgcn_update_dpp(0, iv, 0x124, 0xf, 0xf, true)
                                    : __builtin_amdgcn_update_dpp(0, iv, 0x128, 0xf, 0xf, true);
            v[rt][gq] += __builtin_bit_cast(float, o);
          }
  };
  float sum[RTW][4];
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt))
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float sacc = 0.f;
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const float hv = hreg[rt][TL][gq];
        const float nv = gu_blend(z[rt][TL][gq], hv, tt[rt][TL][gq]);
        tt[rt][TL][gq] = nv;
        sacc += nv;
      }
      sum[rt][gq] = sacc;
    }
  row16_sum_all(sum);
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt))
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        if (a == 0) part[fg * R + 64 * rg + 16 * rt + 4 * q + gq] = sum[rt][gq];
  __syncthreads();
  float mean[RTW][4], inv[RTW][4], var[RTW][4];
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt))
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int rl = 64 * rg + 16 * rt + 4 * q + gq;
      float ms = 0.f;
#pragma unroll
      for (int f2 = 0; f2 < FG; ++f2) ms += part[f2 * R + rl];
      mean[rt][gq] = ms * (1.0f / D);
      float vs = 0.f;
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const float dv = tt[rt][TL][gq] - mean[rt][gq];
        vs = fmaf(dv, dv, vs);
      }
      var[rt][gq] = vs;
    }
  row16_sum_all(var);
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt))
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        if (a == 0) part[FG * R + fg * R + 64 * rg + 16 * rt + 4 * q + gq] = var[rt][gq];
  __syncthreads();
#pragma unroll
  for (int rt = 0; rt < RTW; ++rt)
    if (active(rt))
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int rl = FG * R + 64 * rg + 16 * rt + 4 * q + gq;
      float vs = 0.f;
#pragma unroll
      for (int f2 = 0; f2 < FG; ++f2) vs += part[f2 * R + rl];
      inv[rt][gq] = gu_inv_std(vs, 1.0f / D, p.eps);
    }
  WIDE_STAMP(p.stamps, 7);
  // Every row of the tile (MINI: of its 16-row piece) is stored: the rows past the ion's last are padding of the row
  // space (the gap behind an ion, the rows behind the last one) that nothing reads as a source, a target or a pooled row.
  {
    float* const out = p.h + (row0 + 64 * rg + 4 * q) * D + 16 * fg * NL + a;
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      const int f = 16 * (fg * NL + TL) + a;
      const float gm = bias[3 * D + f], bt = bias[4 * D + f];
#pragma unroll
      for (int rt = 0; rt < RTW; ++rt)
        if (active(rt))
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          out[(16 * rt + gq) * D + 16 * TL] = gu_out(tt[rt][TL][gq], mean[rt][gq], inv[rt][gq], gm, bt, hreg[rt][TL][gq]);
    }
  }
  WIDE_STAMP(p.stamps, 4);
  WIDE_STAMP_REAL(p.stamps, 6);
}

// Grid: tiles_max workgroups, one per 128-row tile of the row space, then 8 x (cus - 1) "mini" workgroups.  The tiles of
// the whole rounds (cus at a time) are updated by their own workgroup; the tiles of the last, partial round - a tile takes
// ~50 us whatever the number of CUs at work - are cut into eight 16-row pieces, one mini workgroup each, so that the round
// costs a third of a tile.  Workgroups are dispatched in grid order: the minis start as the CUs run out of whole tiles.
template <int NT>
__global__ __launch_bounds__(kGuX3Threads, 1) void wide_update_x3b_kernel(GuParams p) {
  extern __shared__ __align__(16) unsigned char smem_b[];
  constexpr int R = kRT3;
  const int end = p.meta[kMetaEnd];
  const int t_live = (end + R - 1) / R;
  const int t_full = p.cus > 0 ? t_live / p.cus * p.cus : t_live;
  const bool split = t_full > 0 && t_full < t_live;  // (a single partial round runs all at once: nothing to gain)
  int tile, sub = -1;
  if ((int)blockIdx.x < p.tiles_max) {
    tile = blockIdx.x;
    if (tile >= t_live || (split && tile >= t_full)) return;
  } else {
    if (!split) return;
    const int m = (int)blockIdx.x - p.tiles_max;
    tile = t_full + (m >> 3);
    sub = m & 7;
    if (tile >= t_live) return;
  }
  const int64_t tile0 = (int64_t)tile * R;
  const int g = (p.n_ions > 1 && tile0 >= p.meta[kMetaBase + 1]) ? 1 : 0;
  const int64_t ion_end = p.meta[kMetaBase + g] + p.meta[kMetaRows + g];
  const int64_t row0 = tile0 + (sub >= 0 ? 16 * sub : 0);
  if (row0 >= ion_end) return;
  if (sub >= 0) x3b_tile<NT, true>(p, row0, g, smem_b);
  else x3b_tile<NT, false>(p, row0, g, smem_b);
}

int launch_wide_update_x3(const GuParams& p, int D, bool big_tiles, int grid, hipStream_t s) {
  if (big_tiles) {  // batches that fill the chip: 128-row tiles
    const size_t lds = gu_x3b_lds_bytes(D);
    if (D == 128) {
      if (int rc = raise_lds<wide_update_x3b_kernel<8>>(lds)) return rc;
      wide_update_x3b_kernel<8><<<grid, kGuX3Threads, lds, s>>>(p);
    } else {
      if (int rc = raise_lds<wide_update_x3b_kernel<4>>(lds)) return rc;
      wide_update_x3b_kernel<4><<<grid, kGuX3Threads, lds, s>>>(p);
    }
    return IMPNN_OK;
  }
  const size_t lds = gu_x3_lds_bytes(D);
  if (D == 128) {
    if (int rc = raise_lds<wide_update_x3_kernel<8>>(lds)) return rc;
    wide_update_x3_kernel<8><<<grid, kGuX3Threads, lds, s>>>(p);
  } else {
    if (int rc = raise_lds<wide_update_x3_kernel<4>>(lds)) return rc;
    wide_update_x3_kernel<4><<<grid, kGuX3Threads, lds, s>>>(p);
  }
  return IMPNN_OK;
}

}  // namespace wide
}  // namespace impnn
