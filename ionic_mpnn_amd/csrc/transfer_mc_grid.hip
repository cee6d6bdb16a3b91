// Monte-Carlo dropout of the transfer head over a cation x anion grid (include/impnn.h: impnn_transfer_mc_grid, _mask,
// _topk, _topk_where): the fourth grid family.
//
// The transfer head has one Dropout, between Dense 128 and Dense 64 (mp_dropout).  A sample s is a thinned head: a row
// m[s] of 128 multipliers (0 where the feature is dropped, 1 / (1 - rate) where it is kept), the same row for every pair
// of the grid - the "fixed set of masks" form of MC dropout - with BatchNormalization on its moving statistics.  All of
// a pair's work up to relu(Dense 128) does not see the mask, so transfer_mc_grid_kernel is transfer_grid_kernel's tile
// (the same u-row staging, dense128_group, prepared image and operand order) with a loop over the samples behind
// Dense 128: the 128 accumulator registers of Dense 128 stay live, a sample forms Dense 64's B operand from them and
// its multipliers, runs Dense 64 and Dense 1 exactly as transfer_grid_kernel does, and leaves its value for the tile's
// 256 pairs in LDS [S][256].  After the last sample thread tid folds pair tid's S values, ascending, into ensemble_stat's
// statistic generalised from 8 to S (mean, population deviation, score = fmaf(kappa, std, mean)) and hands one value
// per pair to the form, as transfer_grid_kernel's res[] does: the stores, the mask words (GridMask), the running top k
// (GridSelect / GridSelectWhere) or the per-ion records (GridSummary), all on the score.  By MFMA count a wave spends 1024 + 256 S where the deterministic
// grid spends 1280.
//
// The multipliers are an operand (S,128); no generator runs here.  They sit in LDS beside the sample array: a lane
// reads the four of a k group with one ds_read_b128 at an address that is the same in each lane half (a broadcast, no
// bank conflict), issued a group ahead with Dense 64's weights.  A pair's S values, and so its statistic, depend on
// its two u rows, the image and the table only - not on the tile, lane, launch, host tiling or the grid's size.  With
// every multiplier 1 a sample has the bits of impnn_transfer_head_grid.  No atomics on floats.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kMcMaxSamples = 64;
constexpr int kMcTilePairs = kTgTileC * kTgTileA;  // 256: a pair per thread
// behind transfer_grid_kernel's regions: the samples' values [S][256] and the multipliers [S][128], 1.5 KiB a sample
__host__ __device__ inline size_t mc_lds_floats(int S) { return kTgLdsFloats + (size_t)S * (kMcTilePairs + kH2); }
// the largest workgroup: the tile's regions, kMcMaxSamples samples, the selecting form's list at k = kSelectMaxK
// (select_capacity(1024, 256) = 2048 entries, select_lds_bytes(1, 2048) = 16 400 bytes) and the _where words
static_assert(sizeof(float) * (kTgLdsFloats + (size_t)kMcMaxSamples * (kMcTilePairs + kH2)) + (2048 * 8 + 16) +
                      sizeof(uint32_t) * kWhereTileWords <= kEnsembleLdsCap,
              "transfer MC grid: kMcMaxSamples samples, the lists and the mask words must fit a CU's LDS");

// What the materialising form writes: any of mean, std, score (C,A) and the sample planes (S,C,A); a null one is skipped.
struct McOut {
  float *mean, *std, *score, *samples;
};

// One k group of Dense 64 on a thinned input: `in` holds relu(Dense 128) already; feature 4 g + b of the block is 0
// where its multiplier is 0 (also for a non-finite activation, as dropout_apply) and relu(a2) * m elsewhere.
__device__ __forceinline__ void dense64_group_mc(f32x16_t (&acc)[2][2], const f32x16_t (&in)[2], const f32x4_t (&w)[2],
                                                 const f32x4_t m, int g) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float a2 = m[b] != 0.f ? in[nb][4 * g + b] * m[b] : 0.f;
      acc[0][nb] = mfma32(w[0][b], a2, acc[0][nb]);
      acc[1][nb] = mfma32(w[1][b], a2, acc[1][nb]);
    }
}

template <class... Sel>
__global__ __launch_bounds__(256) void transfer_mc_grid_kernel(const float* __restrict__ u_cat,
                                                               const float* __restrict__ u_an,
                                                               const float* __restrict__ img,
                                                               const float* __restrict__ mult, McOut out, int S,
                                                               float kappa, int C, int A, int tiles_a, Sel... sel) {
  extern __shared__ __align__(16) float sm[];
  float* uan = sm;                            // [kTgTileA][kTgAnStride]
  float* ucat = uan + kTgTileA * kTgAnStride; // [kTgTileC][kH1]
  float* bnv = ucat + kTgTileC * kH1;         // scale kH1 | shift kH1
  float* res = bnv + 2 * kH1;                 // [kTgTileC][kTgTileA]: the value the form reads
  float* smp = sm + kTgLdsFloats;             // [S][kMcTilePairs]
  float* mul = smp + (size_t)S * kMcTilePairs;  // [S][kH2]
  float* lists = sm + mc_lds_floats(S);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = lane & 31, h = lane >> 5;
  using Form = GridForm<Sel...>;
  static_assert(!Form::partners && !Form::rank_count && !Form::rank_mask, "transfer MC grids: partners / rank are not built");
  constexpr bool kSelect = Form::select;
  unsigned tile = blockIdx.x;
  if constexpr (kSelect) select_init(sel..., lists, 1);
  // the table, once per workgroup (published by the barrier behind the first tile's rows)
  for (int idx = tid; idx < S * (kH2 / 4); idx += blockDim.x)
    *reinterpret_cast<f32x4_t*>(mul + 4 * idx) = ld4(mult + 4 * idx);
  do {
  const int c0 = (tile / tiles_a) * kTgTileC, a0 = (tile % tiles_a) * kTgTileA;
  const int nc = min(kTgTileC, C - c0), na = min(kTgTileA, A - a0);
  if constexpr (Form::where) {  // a tile without a set bit: on to the next one, before any load
    if (!where_tile_any(sel..., lists, 1, c0, nc, a0 >> 5, kTgTileA / 32)) continue;
  }
  if constexpr (Form::summary) {  // the summary form's mask may be null: the same pass, when there is one
    if (summary_masked(sel...) && !where_tile_any(sel..., lists, 1, c0, nc, a0 >> 5, kTgTileA / 32)) {
      summary_skip_tile(sel..., C, A, c0, a0, nc, na, tiles_a, a0 / kTgTileA, (C + kTgTileC - 1) / kTgTileC, c0 / kTgTileC, 1);
      continue;
    }
  }

  // the tile's u rows; the rows of a ragged tile's padding pairs are zero (computed, not stored)
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int idx = tid; idx < kTgTileA * (kH1 / 4); idx += blockDim.x) {
    const int r = idx >> 6, q = idx & 63;
    *reinterpret_cast<f32x4_t*>(uan + r * kTgAnStride + 4 * q) = r < na ? ld4(u_an + (int64_t)(a0 + r) * kH1 + 4 * q) : zero4;
  }
  for (int idx = tid; idx < kTgTileC * (kH1 / 4); idx += blockDim.x) {
    const int r = idx >> 6, q = idx & 63;
    *reinterpret_cast<f32x4_t*>(ucat + r * kH1 + 4 * q) = r < nc ? ld4(u_cat + (int64_t)(c0 + r) * kH1 + 4 * q) : zero4;
  }
  for (int idx = tid; idx < 2 * kH1 / 4; idx += blockDim.x)
    *reinterpret_cast<f32x4_t*>(bnv + 4 * idx) = ld4(img + kImgScale + 4 * idx);
  __syncthreads();

  if (2 * wave < nc) {  // (wave-uniform; no barrier inside)
    const float* ua_row = uan + p * kTgAnStride + 4 * h;
    const float* uc_row = ucat + (2 * wave) * kH1 + 4 * h;
    const f32x4_t* w2 = reinterpret_cast<const f32x4_t*>(img + kImgW2) + lane;

    // Dense 128, as transfer_grid_kernel: bias first, the A operands of k group g + 1 travel under group g's MFMAs
    f32x16_t acc2[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t bb = ld4(img + kImgB2 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc2[mb][0][4 * q + b] = acc2[mb][1][4 * q + b] = bb[b];
      }
    f32x4_t wa[4], wb[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) wa[mb] = w2[mb * 64];
#pragma unroll 1
    for (int g = 0; g < kH1 / 8; g += 2) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) wb[mb] = w2[((g + 1) * 4 + mb) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense128_group(acc2, wa, ua_row, uc_row, bnv + 4 * h, g);
      __builtin_amdgcn_sched_barrier(0);
      const int gn = min(g + 2, kH1 / 8 - 1);  // (the last turn reloads group 31: in bounds, unused)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) wa[mb] = w2[(gn * 4 + mb) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense128_group(acc2, wb, ua_row, uc_row, bnv + 4 * h, g + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    // relu(Dense 128) once for every sample (transfer_grid_kernel applies it where Dense 64 reads the register)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[mb][nb][r] = head_relu(acc2[mb][nb][r]);

    // The samples.  Register 4 g + b of acc2[kb] of lane half h is feature 32 kb + 8 g + 4 h + b: the four multipliers
    // of k group s4 = 4 kb + g are one 16-byte LDS read at ms + 8 s4, the same address in a lane half.
#pragma unroll 1
    for (int smpl = 0; smpl < S; ++smpl) {
      const float* ms = mul + smpl * kH2 + 4 * h;
      // Every sample streams Dense 64's weights, its bias and Dense 1's weights from L2 again, as a tile of
      // transfer_grid_kernel does: hoisted out of this loop they are 200 registers beside acc2's 128 and acc3's 64,
      // which spills.  The empty statement makes the image's address a value of this iteration.
      const float* simg = img;
      asm volatile("" : "+s"(simg));
      const f32x4_t* w3 = reinterpret_cast<const f32x4_t*>(simg + kImgW3) + lane;
      // Dense 64: bias first, the k-ordered chain of transfer_grid_kernel
      f32x16_t acc3[2][2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4_t bb = ld4(simg + kImgB3 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
          for (int b = 0; b < 4; ++b) acc3[mb][0][4 * q + b] = acc3[mb][1][4 * q + b] = bb[b];
        }
      f32x4_t va[2], vb[2], ma, mb4;
      va[0] = w3[0], va[1] = w3[64], ma = ld4(ms);
#pragma unroll
      for (int s = 0; s < 16; s += 2) {  // s = 4 kb + g
        vb[0] = w3[((s + 1) * 2 + 0) * 64], vb[1] = w3[((s + 1) * 2 + 1) * 64], mb4 = ld4(ms + 8 * (s + 1));
        __builtin_amdgcn_sched_barrier(0);
        dense64_group_mc(acc3, acc2[s >> 2], va, ma, s & 3);
        __builtin_amdgcn_sched_barrier(0);
        const int sn = s + 2 < 16 ? s + 2 : 15;
        va[0] = w3[(sn * 2 + 0) * 64], va[1] = w3[(sn * 2 + 1) * 64], ma = ld4(ms + 8 * sn);
        __builtin_amdgcn_sched_barrier(0);
        dense64_group_mc(acc3, acc2[(s + 1) >> 2], vb, mb4, (s + 1) & 3);
        __builtin_amdgcn_sched_barrier(0);
      }

      // Dense 1: a lane sums its 32 features in ascending order, the two lane halves meet (half 0 first), then the bias
      float part[2] = {0.f, 0.f};
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4_t wo = ld4(simg + kImgWo + 32 * mb + 8 * q + 4 * h);
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) part[nb] = fmaf(head_relu(acc3[mb][nb][4 * q + b]), wo[b], part[nb]);
        }
      const float bo = simg[kImgBo];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float other = __shfl_xor(part[nb], 32);
        if (h == 0) smp[smpl * kMcTilePairs + (2 * wave + nb) * kTgTileA + p] = (part[nb] + other) + bo;
      }
    }
  }
  __syncthreads();

  // The statistic of pair tid (row tid >> 5, anion tid & 31) in float32 and in this order (ensemble_stat's, for S):
  //   s = v_0; s = s + v_i (i ascending); mean = s / S
  //   q = 0; d = v_i - mean; q = fmaf(d, d, q) (i ascending); std = sqrt(q / S)      (the population deviation)
  //   score = fmaf(kappa, std, mean)
  // (a pair outside the grid, or of a row no wave computed: stale LDS, never stored, never live)
  float sum = smp[tid];
  for (int i = 1; i < S; ++i) sum = sum + smp[i * kMcTilePairs + tid];
  const float n = (float)S, mean = sum / n;
  float q = 0.f;
  for (int i = 0; i < S; ++i) {
    const float d = smp[i * kMcTilePairs + tid] - mean;
    q = fmaf(d, d, q);
  }
  const float sd = sqrtf(q / n), score = fmaf(kappa, sd, mean);

  if constexpr (kSelect) {
    res[tid] = score;
    __syncthreads();
    select_tile(sel..., lists, 1, kMcTilePairs, [&](int, int, bool* live, uint32_t* pair) {
      const int r = tid >> 5;
      *live = r < nc && p < na;
      if constexpr (Form::where) *live = *live && where_bit(sel..., lists, 1, r, p, kTgTileA / 32);
      *pair = (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + p);
      return res[tid];
    });
  } else if constexpr (Form::mask) {
    // a wave's lanes are two tile rows of 32 anions: lane 0 and lane 32 each write the word of their own row
    const int r = tid >> 5;
    uint32_t* word = mask_word(sel..., c0 + r, a0 >> 5);
    mask_store_ballot(r < nc && p < na && mask_passes(sel..., score), r < nc ? word : nullptr, r < nc ? word : nullptr);
  } else if constexpr (Form::summary) {
    res[tid] = score;
    __syncthreads();
    summary_transfer_tile(sel..., res, C, A, c0, a0, nc, na, tiles_a, [&](int r, int a) {
      return !summary_masked(sel...) || where_bit(sel..., lists, 1, r, a, kTgTileA / 32);
    });
  } else {
    const int64_t first = (int64_t)c0 * A + a0;
    float* const outs[3] = {out.mean, out.std, out.score};
    const float vals[3] = {mean, sd, score};
#pragma unroll
    for (int o = 0; o < 3; ++o)
      if (outs[o]) {  // (block-uniform: a kernel argument)
        res[tid] = vals[o];
        __syncthreads();
        store_spans(outs[o], first, (int64_t)A, nc, na, res, kTgTileA);
        __syncthreads();
      }
    if (out.samples)
      for (int i = 0; i < S; ++i)
        store_spans(out.samples + (int64_t)i * C * A, first, (int64_t)A, nc, na, smp + i * kMcTilePairs, kTgTileA);
  }
  } while (select_next_tile(&tile, sel...));  // (the materialising and mask forms: one tile per workgroup)
  if constexpr (kSelect) select_finish(sel..., lists, 1);
}

// every launch of the kernel: `groups` workgroups, `extra_lds` bytes behind the samples and the table, the form's pack
template <class... Sel>
void launch_mc(const GridOperands& g, unsigned groups, size_t extra_lds, const McOut& out, Sel... sel) {
  const size_t lds = sizeof(float) * mc_lds_floats(g.M) + extra_lds;
  auto kern = transfer_mc_grid_kernel<Sel...>;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<groups, 256, lds, g.stream>>>(g.mix_cat, g.mix_an, g.w, g.multipliers, out, g.M, g.kappa, g.C, g.A,
                                       grid_tiles(3, g.C, g.A).a, sel...);
}

}  // namespace

int transfer_mc_grid_max_samples() { return kMcMaxSamples; }

int launch_transfer_mc_grid(const GridOperands& g, float* mean, float* std, float* score, float* samples) {
  const GridTiles tiles = grid_tiles(3, g.C, g.A);
  if (int rc = grid_tiles_fit("transfer_mc_grid", tiles)) return rc;
  launch_mc(g, (unsigned)tiles.count(), 0, McOut{mean, std, score, samples});
  return check_launch("transfer_mc_grid");
}

int launch_transfer_mc_grid_mask(const GridMaskCall& c) {
  const GridTiles tiles = grid_tiles(3, c.g.C, c.g.A);
  if (int rc = grid_tiles_fit("transfer_mc_grid_mask", tiles)) return rc;
  launch_mc(c.g, (unsigned)tiles.count(), 0, McOut{}, GridMask{c.words, c.lo, c.hi, mask_row_words(c.g.A)});
  return check_launch("transfer_mc_grid_mask");
}

// the tile launch of a summary call (grid_summary.hip merges the partial records): the mask words behind the samples
void launch_transfer_mc_grid_summary_tiles(const GridOperands& g, unsigned groups, const GridSummary& sel) {
  launch_mc(g, groups, sizeof(uint32_t) * kWhereTileWords, McOut{}, sel);
}

int launch_transfer_mc_grid_topk(const GridTopkCall& c) {
  const GridOperands& g = c.g;
  const int64_t tiles = grid_tiles(3, g.C, g.A).count();
  const int G = grid_topk_workgroups(3, g.C, g.A, c.workgroups);
  const int cap = select_capacity(c.k, kMcTilePairs);
  unsigned long long* ws = static_cast<unsigned long long*>(c.workspace);
  const GridSelect sel{ws, c.k, cap, c.largest, (unsigned)tiles};
  const size_t sel_lds = select_lds_bytes(1, cap);  // behind the samples and the table; api.hip holds S to what fits
  if (c.masked) {
    GridSelectWhere selw;
    static_cast<GridSelect&>(selw) = sel;
    selw.where = c.where, selw.W = mask_row_words(g.A);
    launch_mc(g, G, sel_lds + sizeof(uint32_t) * kWhereTileWords, McOut{}, selw);
  } else {
    launch_mc(g, G, sel_lds, McOut{}, sel);
  }
  if (int rc = check_launch("transfer_mc_grid_topk")) return rc;
  return launch_grid_topk_merge(ws, G, 1, c.k, c.largest, g.A, c.values, c.cation, c.anion, g.stream);
}

}  // namespace impnn
