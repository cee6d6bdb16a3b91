// The exact-f32 GatedUpdate of the wide encoder (encoder_wide.hip has the stage list): wide_update on 64-row tiles
// (or the 32 rows GuParams::tile_rows asks for) and wide_update_small on 16-row tiles.
#include "wide_device.h"

namespace impnn {
namespace wide {

// a7 on kRT-row tiles of the compact row space, h updated in place.  8 waves per tile, TWO workgroups resident per CU
// (77 KB of LDS and 128 VGPRs each): exact-f32 MFMA and the vector ALU share one issue port, so a tile's barrier
// bubbles, its prologue and its LayerNorm epilogue are only ever hidden by ANOTHER tile's MFMAs.
//   phase 1   [z|r] pre-activations = [h|agg] (R x 2D) x [Wz|Wr] (2D x 2D): 2 NT slices of 16 k; a slice of the rows
//             (4 KB, MFMA operand order [k quad][row][4]) and of the kernels (16 KB at D = 128, the image's own order)
//             goes global -> registers (two slices ahead) -> one of two LDS stages; one barrier per slice, 32 MFMAs
//             per wave between barriers (wave = 32 rows x NL feature tiles of z and of r).
//   phase 2   candidate = [r*h|agg] x Wh, 2 NT slices again: r*h comes from LDS (written once after phase 1), agg and
//             Wh through the stages.
//   epilogue  blend, LayerNorm (row sums across the four feature groups through LDS), residual.
// h of the accumulator positions is read once into registers (for r*h, the blend and the residual).
constexpr int kGuThreads = 512;
constexpr size_t gu_lds_floats(int D) {
  // two stages of (row slice + [Wz|Wr] slice) | r*h | LayerNorm partials
  return 2 * (size_t)(4 * kRT * 4 + 4 * 2 * D * 4) + (size_t)kRT * (D + 4) + 8 * kRT;
}

template <int NT>
__global__ __launch_bounds__(kGuThreads, 4) void wide_update_kernel(GuParams p) {
  constexpr int D = 16 * NT, R = kRT, LDR = D + 4;
  constexpr int RG = R / 32, FG = (kGuThreads / 64) / RG, NL = NT / FG;
  constexpr int A1 = 4 * R * 4;       // floats of a 16-k slice of the rows
  constexpr int B1 = 4 * 2 * D * 4;   // ... of [Wz|Wr]
  constexpr int B2 = 4 * D * 4;       // ... of Wh
  constexpr int ST = A1 + B1;         // stage floats
  constexpr int kQ1 = (B1 / 4 + kGuThreads - 1) / kGuThreads, kQ2 = (B2 / 4 + kGuThreads - 1) / kGuThreads;
  constexpr int kAT = R * 4;          // threads that move a piece of a row slice
  static_assert(NL >= 1 && NT % FG == 0 && kAT <= kGuThreads, "tile shape");
  extern __shared__ __align__(16) float smem[];
  float* stage = smem;                 // 2 x ST
  float* rhs = stage + 2 * ST;         // R x LDR : r * h
  float* part = rhs + R * LDR;         // 2 x FG x R LayerNorm partials
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, a = lane & 15, q = lane >> 4;
  const int rg = wv % RG, fg = wv / RG;  // row group (32 rows), feature group (NL tiles of z, r and the candidate)
  // A workgroup's LDS tile always spans R rows; with tile_rows < R only its first tile_rows rows are the workgroup's
  // own (the rest is read like any padding and never stored), and the 16-row tiles past them are not multiplied:
  // 768 64-row tiles on 512 slots are two rounds, the second half empty - 1 536 32-row tiles are three short ones.
  const int64_t row0 = (int64_t)blockIdx.x * p.tile_rows;
  const int end = p.meta[kMetaEnd];
  if (row0 >= end) return;
  const int g = (p.n_ions > 1 && row0 >= p.meta[kMetaBase + 1]) ? 1 : 0;
  const int64_t ion_end = p.meta[kMetaBase + g] + p.meta[kMetaRows + g];
  const int64_t row_end = row0 + p.tile_rows < ion_end ? row0 + p.tile_rows : ion_end;  // rows beyond it are not this tile's
  if (row0 >= row_end) return;
  const bool lv[2] = {32 * rg < p.tile_rows, 32 * rg + 16 < p.tile_rows};  // (wave-uniform) this wave's two row tiles
  WIDE_STAMP(p.stamps, 0);
  WIDE_STAMP_REAL(p.stamps, 5);
  const float* img = p.img[g] + p.gu_off;
  const float* P1 = img;
  const float* P2 = img + 4 * D * D;
  const float* bias = img + 6 * D * D;  // bz br bh gamma beta
  // (padding rows of the last tile of an ion lie inside the workspace; whatever they hold stays in their own rows)
  const int a_row = (tid % kAT) >> 2, a_c4 = tid & 3;
  const float* hsrc = p.h + (row0 + a_row) * D + 4 * a_c4;
  // the row's aggregated messages: two sources (wide_iota_kernel), as float offsets from p.agg
  const int goff0 = agg_off(p.c2a[row0 + a_row], p.m_off, D) + 4 * a_c4, goff1 = agg_off(p.c2b[row0 + a_row], p.m_off, D) + 4 * a_c4;
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  struct Pre {
    f32x4_t av, aw, bv[kQ1];  // aw: the second source of a slice of aggregated messages (zeros for a slice of h)
  };
  Pre preA, preB;
  auto fetch1 = [&](int u, Pre& pre) {
#pragma unroll
    for (int i = 0; i < kQ1; ++i)
      if (tid + kGuThreads * i < B1 / 4) pre.bv[i] = ldv4(P1 + (size_t)u * B1 + (tid + kGuThreads * i) * 4);
#ifdef IMPNN_DIAG_WIDE_NOFETCH
    if (tid < kAT) { pre.av = f32x4_t{0.25f, 0.5f, -0.25f, 0.125f}; pre.aw = zero4; }
#else
    if (tid < kAT) {
      if (u < NT) {  // (workgroup-uniform)
        pre.av = ldv4(hsrc + 16 * u);
        pre.aw = zero4;
      } else {
        pre.av = ldv4(p.agg + goff0 + 16 * (u - NT));
        pre.aw = ldv4(p.agg + goff1 + 16 * (u - NT));
      }
    }
#endif
  };
  auto park1 = [&](float* st, const Pre& pre) {
#pragma unroll
    for (int i = 0; i < kQ1; ++i)
      if (tid + kGuThreads * i < B1 / 4) stv4(st + A1 + (tid + kGuThreads * i) * 4, pre.bv[i]);
    if (tid < kAT) stv4(st + (a_c4 * R + a_row) * 4, pre.av + pre.aw);  // (first slot first: the Reduce's order)
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
  struct Ops1 {
    f32x4_t av[2], bz[NL], br[NL];
  };
  auto read1 = [&](const float* st, Ops1& o) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) o.av[rt] = ldv4(st + (q * R + 32 * rg + 16 * rt + a) * 4);
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      o.bz[TL] = ldv4(st + A1 + (q * 2 * D + 16 * (fg * NL + TL) + a) * 4);
      o.br[TL] = ldv4(st + A1 + (q * 2 * D + D + 16 * (fg * NL + TL) + a) * 4);
    }
  };
  auto mma1 = [&](const Ops1& o) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      if (lv[rt]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int TL = 0; TL < NL; ++TL) {
            z[rt][TL] = mfma_f32(o.av[rt][r], o.bz[TL][r], z[rt][TL]);
            rr[rt][TL] = mfma_f32(o.av[rt][r], o.br[TL][r], rr[rt][TL]);
          }
      }
  };
  fetch1(0, preA);
  fetch1(1, preB);
  park1(stage, preA);
  __syncthreads();
  WIDE_STAMP(p.stamps, 1);
  // h at this lane's accumulator positions (rows 4q + g of both row tiles, feature a of its NL tiles): requested under
  // the last two slices of phase 1 - held from the start they cost 16 registers the phase does not have
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
  // iteration u: slice u is in stage u & 1, slice u + 1 in registers, slice u + 2 is requested; stage (u + 1) & 1 was
  // last read in iteration u - 1, whose closing barrier every wave has passed
  auto pair1 = [&](int u) {
    Ops1 o;
    if (u + 2 < 2 * NT) fetch1(u + 2, preA);
    read1(stage, o);
    __builtin_amdgcn_sched_barrier(0);
    park1(stage + ST, preB);
    __builtin_amdgcn_sched_barrier(0);
    mma1(o);
    __syncthreads();
    if (u + 3 < 2 * NT) fetch1(u + 3, preB);
    read1(stage + ST, o);
    __builtin_amdgcn_sched_barrier(0);
    if (u + 2 < 2 * NT) park1(stage, preA);
    __builtin_amdgcn_sched_barrier(0);
    mma1(o);
    __syncthreads();
  };
  for (int u = 0; u < 2 * NT - 2; u += 2) pair1(u);
  load_hreg();
  pair1(2 * NT - 2);
  WIDE_STAMP(p.stamps, 2);
  // ---- phase 2
  struct Pre2 {
    f32x4_t av, aw, bv[kQ2];
  };
  Pre2 qA, qB;
  auto fetch2 = [&](int u, Pre2& pre) {
#pragma unroll
    for (int i = 0; i < kQ2; ++i)
      if (tid + kGuThreads * i < B2 / 4) pre.bv[i] = ldv4(P2 + (size_t)u * B2 + (tid + kGuThreads * i) * 4);
#ifdef IMPNN_DIAG_WIDE_NOFETCH
    if (u >= NT && tid < kAT) { pre.av = f32x4_t{0.25f, 0.5f, -0.25f, 0.125f}; pre.aw = zero4; }
#else
    if (u >= NT && tid < kAT) {
      pre.av = ldv4(p.agg + goff0 + 16 * (u - NT));
      pre.aw = ldv4(p.agg + goff1 + 16 * (u - NT));
    }
#endif
  };
  auto park2 = [&](int u, float* st, const Pre2& pre) {
#pragma unroll
    for (int i = 0; i < kQ2; ++i)
      if (tid + kGuThreads * i < B2 / 4) stv4(st + A1 + (tid + kGuThreads * i) * 4, pre.bv[i]);
    if (u >= NT && tid < kAT) stv4(st + (a_c4 * R + a_row) * 4, pre.av + pre.aw);
  };
  fetch2(0, qA);
  fetch2(1, qB);
  // gates; r * h into LDS (phase 2 reads the rows of this wave's row group written by all feature groups)
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
  park2(0, stage, qA);
  __syncthreads();
  struct Ops2 {
    f32x4_t av[2], bv[NL];
  };
  auto read2 = [&](int u, const float* st, Ops2& o) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      o.av[rt] = u < NT ? ldv4(rhs + (32 * rg + 16 * rt + a) * LDR + 16 * u + 4 * q)
                        : ldv4(st + (q * R + 32 * rg + 16 * rt + a) * 4);
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) o.bv[TL] = ldv4(st + A1 + (q * D + 16 * (fg * NL + TL) + a) * 4);
  };
  auto mma2 = [&](const Ops2& o) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
      if (lv[rt]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int TL = 0; TL < NL; ++TL) tt[rt][TL] = mfma_f32(o.av[rt][r], o.bv[TL][r], tt[rt][TL]);
      }
  };
  for (int u = 0; u < 2 * NT; u += 2) {
    Ops2 o;
    if (u + 2 < 2 * NT) fetch2(u + 2, qA);
    read2(u, stage, o);
    __builtin_amdgcn_sched_barrier(0);
    park2(u + 1, stage + ST, qB);
    __builtin_amdgcn_sched_barrier(0);
    mma2(o);
    __syncthreads();
    if (u + 3 < 2 * NT) fetch2(u + 3, qB);
    read2(u + 1, stage + ST, o);
    __builtin_amdgcn_sched_barrier(0);
    if (u + 2 < 2 * NT) park2(u + 2, stage, qA);
    __builtin_amdgcn_sched_barrier(0);
    mma2(o);
    __syncthreads();
  }
  WIDE_STAMP(p.stamps, 3);
  // ---- blend, LayerNorm over the D features of a row, residual (models/layers.py:150-156)
  // (row sums over the 16 lanes of a quarter wave, all of the wave's rows step by step: a row's next DPP step is eight
  //  instructions behind its last, no stall between dependent DPP operations)
  auto row16_sum_all = [&](float (&v)[2][4]) {
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
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
      sum[rt][gq] = sacc;
    }
  row16_sum_all(sum);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      if (a == 0) part[fg * R + 32 * rg + 16 * rt + 4 * q + gq] = sum[rt][gq];
  __syncthreads();
  float mean[2][4], inv[2][4], var[2][4];
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
      var[rt][gq] = vs;
    }
  row16_sum_all(var);
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      if (a == 0) part[FG * R + fg * R + 32 * rg + 16 * rt + 4 * q + gq] = var[rt][gq];
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
  {
    float* const out = p.h + (row0 + 32 * rg + 4 * q) * D + 16 * fg * NL + a;
    // a whole tile (tile_rows == R) stores every row: rows past row_end are padding of the row space, which nothing
    // reads as a source, a target or a pooled row; a workgroup that owns only the first rows of its LDS tile checks
    const bool all_rows = p.tile_rows == R;  // (workgroup-uniform)
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      const int f = 16 * (fg * NL + TL) + a;
      const float gm = bias[3 * D + f], bt = bias[4 * D + f];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const float v = gu_out(tt[rt][TL][gq], mean[rt][gq], inv[rt][gq], gm, bt, hreg[rt][TL][gq]);
          if (all_rows || row0 + 32 * rg + 16 * rt + 4 * q + gq < row_end) out[(16 * rt + gq) * D + 16 * TL] = v;
        }
    }
  }
  WIDE_STAMP(p.stamps, 4);
  WIDE_STAMP_REAL(p.stamps, 6);
}

// ------------------------------------------------------------------------------------------------------------
// a7 for launches too small to fill the chip (16-row tiles: batches of up to ~100 pairs - model.predict at the
// reference's batch 32).  There wide_update_kernel is a chain of 32 weight slices through LDS with a barrier each:
// 29 us per launch whatever the rows, half of the forward's latency.  Here a 4-wave workgroup owns 16 rows, wave w the
// features [w D/4, (w + 1) D/4) of z, r and the candidate, and every operand comes straight from global memory / L2 in
// 16-byte pieces - the kernels in the prepared image's own order ([16-k slice][k quad][column][4 k]: a lane's four k of
// a slice are one load, MFMA step r takes component r of both operands), the rows' h from an LDS copy, the
// aggregated messages from their two sources - three slices ahead of the MFMAs: no staging, four barriers per tile.
// Exact f32 (v_mfma_f32_16x16x4_f32), the products and their order per output as wide_update_kernel's.
// ------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT >= 8 ? 512 : 256) void wide_update_small_kernel(GuParams p) {
  // WV waves: wave w owns the features [w D / WV, (w + 1) D / WV) - one 16-feature tile at D = 128 (8 waves), at D = 64 (4)
  constexpr int WV = NT >= 8 ? 8 : 4, T = 64 * WV;
  constexpr int D = 16 * NT, NL = NT / WV, LDH = D + 4, R = 16, NS = NT;  // NS 16-k slices per D of contraction
  static_assert(NL >= 1, "tile shape");
  __shared__ __align__(16) float hs[R * LDH];   // h of the tile's rows
  __shared__ __align__(16) float rhs[R * LDH];  // r * h
  __shared__ float part[2][4][R];               // LayerNorm partials: [sum | squared deviations][feature group][row]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, a = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int end = p.meta[kMetaEnd];
  if (row0 >= end) return;
  const int g = (p.n_ions > 1 && row0 >= p.meta[kMetaBase + 1]) ? 1 : 0;
  const int64_t ion_end = p.meta[kMetaBase + g] + p.meta[kMetaRows + g];
  const int64_t row_end = row0 + R < ion_end ? row0 + R : ion_end;
  if (row0 >= row_end) return;
  const float* img = p.img[g] + p.gu_off;
  const f32x4_t* P1 = reinterpret_cast<const f32x4_t*>(img);              // [Wz|Wr]: unit ((u * 4 + qq) * 2D + column)
  const f32x4_t* P2 = reinterpret_cast<const f32x4_t*>(img + 4 * D * D);  // Wh: unit ((u * 4 + qq) * D + column)
  const float* bias = img + 6 * D * D;                                    // bz br bh gamma beta
  for (int i = tid; i < R * D / 4; i += T) {
    const int r = i / (D / 4), c4 = i - r * (D / 4);
    stv4(hs + r * LDH + 4 * c4, ldv4(p.h + (row0 + r) * D + 4 * c4));
  }
  // the aggregated messages of the lane's row (A operand: row a, k = 4 q .. 4 q + 3 of a slice): two sources
  const int goff0 = agg_off(p.c2a[row0 + a], p.m_off, D) + 4 * q, goff1 = agg_off(p.c2b[row0 + a], p.m_off, D) + 4 * q;
  const int f0 = 16 * (wv * NL) + a;  // the lane's column of the wave's first feature tile
  f32x4_t z[NL], rr[NL], tt[NL];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const float b0 = bias[f0 + 16 * TL], b1 = bias[D + f0 + 16 * TL], b2 = bias[2 * D + f0 + 16 * TL];
    z[TL] = f32x4_t{b0, b0, b0, b0};
    rr[TL] = f32x4_t{b1, b1, b1, b1};
    tt[TL] = f32x4_t{b2, b2, b2, b2};
  }
  __syncthreads();
  struct Ops {
    f32x4_t av, aw, bz[NL], br[NL];
  };
  constexpr int kAhead = 3;
  // ---- phase 1: [z|r] pre-activations = [h|agg] x [Wz|Wr]
  {
    Ops o[kAhead];
    auto load1 = [&](int u, Ops& x) {
      if (u < NS) {
        x.av = ldv4(hs + a * LDH + 16 * u + 4 * q);
        x.aw = f32x4_t{0.f, 0.f, 0.f, 0.f};
      } else {
        x.av = ldv4(p.agg + goff0 + 16 * (u - NS));
        x.aw = ldv4(p.agg + goff1 + 16 * (u - NS));
      }
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        x.bz[TL] = P1[(u * 4 + q) * 2 * D + f0 + 16 * TL];
        x.br[TL] = P1[(u * 4 + q) * 2 * D + D + f0 + 16 * TL];
      }
    };
#pragma unroll
    for (int u = 0; u < kAhead - 1; ++u) load1(u, o[u]);
#pragma unroll
    for (int u = 0; u < 2 * NS; ++u) {
      if (u + kAhead - 1 < 2 * NS) load1(u + kAhead - 1, o[(u + kAhead - 1) % kAhead]);
      __builtin_amdgcn_sched_barrier(0);  // (the requests stay in front of this slice's MFMAs)
      const Ops& x = o[u % kAhead];
      const f32x4_t av = x.av + x.aw;  // (first slot first: the Reduce's order; h + 0 for a slice of h)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int TL = 0; TL < NL; ++TL) {
          z[TL] = mfma_f32(av[r], x.bz[TL][r], z[TL]);
          rr[TL] = mfma_f32(av[r], x.br[TL][r], rr[TL]);
        }
    }
  }
  // ---- gates; r * h into LDS (accumulator layout: column a of the tile, rows 4 q + i)
#pragma unroll
  for (int TL = 0; TL < NL; ++TL)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      z[TL][i] = fsig(z[TL][i]);
      rhs[(4 * q + i) * LDH + f0 + 16 * TL] = gu_rh(rr[TL][i], hs[(4 * q + i) * LDH + f0 + 16 * TL]);
    }
  __syncthreads();
  // ---- phase 2: candidate = [r * h|agg] x Wh
  {
    struct Ops2 {
      f32x4_t av, aw, bh[NL];
    };
    Ops2 o[kAhead];
    auto load2 = [&](int u, Ops2& x) {
      if (u < NS) {
        x.av = ldv4(rhs + a * LDH + 16 * u + 4 * q);
        x.aw = f32x4_t{0.f, 0.f, 0.f, 0.f};
      } else {
        x.av = ldv4(p.agg + goff0 + 16 * (u - NS));
        x.aw = ldv4(p.agg + goff1 + 16 * (u - NS));
      }
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) x.bh[TL] = P2[(u * 4 + q) * D + f0 + 16 * TL];
    };
#pragma unroll
    for (int u = 0; u < kAhead - 1; ++u) load2(u, o[u]);
#pragma unroll
    for (int u = 0; u < 2 * NS; ++u) {
      if (u + kAhead - 1 < 2 * NS) load2(u + kAhead - 1, o[(u + kAhead - 1) % kAhead]);
      __builtin_amdgcn_sched_barrier(0);
      const Ops2& x = o[u % kAhead];
      const f32x4_t av = x.av + x.aw;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int TL = 0; TL < NL; ++TL) tt[TL] = mfma_f32(av[r], x.bh[TL][r], tt[TL]);
    }
  }
  // ---- blend, LayerNorm over the D features of a row, residual.  The partial sums are formed exactly as
  // wide_update_kernel forms them - per feature GROUP of D / 4 features: lane-wise over the group's tiles, then over the
  // 16 lanes, then over the four groups - so that a batch and its chunks agree bit for bit whichever kernel they take.
  // With 8 waves (D = 128) a group is two waves: the odd one hands its blended values to the even one through LDS.
  constexpr bool kPair = WV == 8;
  constexpr int NG = kPair ? 2 : NL;  // tiles of a feature group as the summing wave sees them
  static_assert(!kPair || NL == 1, "pairs of single-tile waves");
  float hv[NL][4];
#pragma unroll
  for (int TL = 0; TL < NL; ++TL)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hv[TL][i] = hs[(4 * q + i) * LDH + f0 + 16 * TL];
      tt[TL][i] = gu_blend(z[TL][i], hv[TL][i], tt[TL][i]);
    }
  float grp[NG][4];  // the group's blended values at this lane's positions
#pragma unroll
  for (int i = 0; i < 4; ++i) grp[0][i] = tt[0][i];  // (an odd wave of a pair does not sum: its copy goes through LDS)
  if (!kPair) {
#pragma unroll
    for (int TL = 1; TL < NL; ++TL)
#pragma unroll
      for (int i = 0; i < 4; ++i) grp[TL < NG ? TL : 0][i] = tt[TL][i];
  } else {
    float* xch = rhs;  // (r * h is dead: every wave is past phase 2's reads only after the barrier below)
    __syncthreads();
    if (wv & 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) xch[((wv >> 1) * 4 + i) * 64 + lane] = tt[0][i];
    }
    __syncthreads();
    if (!(wv & 1)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) grp[1][i] = xch[((wv >> 1) * 4 + i) * 64 + lane];
    }
  }
  const bool summing = !kPair || !(wv & 1);  // (wave-uniform)
  const int fgi = kPair ? wv >> 1 : wv;      // feature group
  if (summing) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float sacc = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < NG; ++t2) sacc += grp[t2][i];
      const float sm = row16_sum_f(sacc);
      if (a == 0) part[0][fgi][4 * q + i] = sm;
    }
  }
  __syncthreads();
  float mean[4], inv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = 4 * q + i;
    float ms = 0.f;
#pragma unroll
    for (int f2 = 0; f2 < 4; ++f2) ms += part[0][f2][rl];
    mean[i] = ms * (1.0f / D);
    if (summing) {
      float vs = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < NG; ++t2) {
        const float dv = grp[t2][i] - mean[i];
        vs = fmaf(dv, dv, vs);
      }
      const float vr = row16_sum_f(vs);
      if (a == 0) part[1][fgi][rl] = vr;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = 4 * q + i;
    float vs = 0.f;
#pragma unroll
    for (int f2 = 0; f2 < 4; ++f2) vs += part[1][f2][rl];
    inv[i] = gu_inv_std(vs, 1.0f / D, p.eps);
  }
#pragma unroll
  for (int TL = 0; TL < NL; ++TL) {
    const int f = f0 + 16 * TL;
    const float gm = bias[3 * D + f], bt = bias[4 * D + f];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = row0 + 4 * q + i;
      if (row < row_end) p.h[row * D + f] = gu_out(tt[TL][i], mean[i], inv[i], gm, bt, hv[TL][i]);
    }
  }
}

int launch_wide_update(const GuParams& p, int D, int grid, hipStream_t s) {
  if (p.tile_rows == 16) {  // launches too small to fill the chip
    if (D == 128) wide_update_small_kernel<8><<<grid, 512, 0, s>>>(p);
    else wide_update_small_kernel<4><<<grid, 256, 0, s>>>(p);
    return IMPNN_OK;
  }
  const size_t lds = gu_lds_floats(D) * 4;
  if (D == 128) {
    if (int rc = raise_lds<wide_update_kernel<8>>(lds)) return rc;
    wide_update_kernel<8><<<grid, kGuThreads, lds, s>>>(p);
  } else {
    if (int rc = raise_lds<wide_update_kernel<4>>(lds)) return rc;
    wide_update_kernel<4><<<grid, kGuThreads, lds, s>>>(p);
  }
  return IMPNN_OK;
}

}  // namespace wide
}  // namespace impnn
