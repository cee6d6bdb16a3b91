// A diverse batch of k pairs by farthest-point (k-center greedy) selection in the latent space (include/impnn.h:
// impnn_diverse_select).  The state is a (C, A) float32 plane of each pair's distance to the reference set plus the
// pairs chosen so far - the value impnn_domain_grid would write against those rows - NaN for a pair that does not
// compete (mask bit clear, NaN vector), so "candidate" is D > 0 and the mask is read once.
//
//   init    the domain grid kernel's scan (domain_device.h: the same bits) -> the plane, the number of candidates, one
//           flag per 16 x 64 tile "no candidate here", and pick 0
//   step t  reads pick t - 1 from the record array, D = min(D, dist(z, z(pick))) for the tile, and reduces pick t
//   decode  records -> cation, anion, distance, n
//
// A pick is the maximum of a 64-bit key, distance bits high (positive floats order as their bits), complemented pair
// index low (the lowest i * A + j wins among equal distances): across the wave by shuffles, across the workgroup
// through LDS, then one 64-bit atomicMax per workgroup into slot t of the zeroed record array (one of the slot's 64
// sub-slots, see below) - a vector global atomic of an order-independent operation, so the result does not depend on the
// schedule.  Key 0 is "no pick": a launch that finds slot t - 1 empty returns at once, the selection has ended.  No host
// synchronisation between the launches.
//
// The step keeps the domain kernels' tile and lane = anion, a thread has four tile rows: one anion-row read serves
// four pairs, the cation rows and the chosen vector are broadcasts.  The plane goes through an LDS tile so that global
// memory sees 16 bytes per lane where A is a multiple of 4 (the plane is 16-byte aligned), 4 bytes otherwise.
#include "domain_device.h"

namespace impnn {
namespace {

// A step's slot is kDiverseSubSlots keys, 64 bytes apart, and a pick the maximum over them: workgroup b lands in sub-slot
// b % kDiverseSubSlots.  Atomics execute at the memory side in 64-byte requests and those to one address queue up: with
// one key per step a 4 096 x 4 096 grid's 16 384 workgroups took 199 us a step, with 64 sub-slots 83 us.
constexpr int kDiverseSubSlots = 64, kDiverseSubStride = 8;  // (in 64-bit words)
constexpr int kDiverseSlotWords = kDiverseSubSlots * kDiverseSubStride;

// the workspace, carved by diverse_carve: the slots of k steps and, behind them, the candidate count
struct DiverseState {
  float* plane;                 // (C, A)
  unsigned long long* records;  // [k * kDiverseSlotWords + 1]
  uint32_t* flags;              // [tiles]: 1 = no candidate in the tile
};

__device__ __forceinline__ unsigned long long* diverse_sub_slot(const DiverseState& st, int t, int sub) {
  return st.records + (size_t)t * kDiverseSlotWords + (size_t)sub * kDiverseSubStride;
}

// the reduction's scratch and the tile's mask words, behind a kernel's float regions (16-byte aligned)
struct DiverseScratch {
  unsigned long long key[4];
  uint32_t count[4];
  uint32_t words[kWhereTileWords];
};

__device__ __forceinline__ unsigned long long diverse_key(float d, uint32_t pair) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)~pair;
}

__device__ __forceinline__ unsigned long long diverse_wave_max(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = __shfl_xor(x, off);
    x = y > x ? y : x;
  }
  return x;
}

// The workgroup's best key into slot `slot`; returns (to thread 0) whether the tile holds a candidate.  Every thread
// calls it; wave-uniform control flow.
__device__ __forceinline__ bool diverse_offer(DiverseScratch* sc, unsigned long long key, unsigned long long* slot) {
  key = diverse_wave_max(key);
  if ((threadIdx.x & 63) == 0) sc->key[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int w = 1; w < 4; ++w) key = sc->key[w] > key ? sc->key[w] : key;
  if (key != 0) atomicMax(slot, key);
  return key != 0;
}

// Pick t, in every lane of the calling wave: lane = sub-slot (kDiverseSubSlots is a wave).  0: no pick.
__device__ __forceinline__ unsigned long long diverse_pick(const DiverseState& st, int t) {
  return diverse_wave_max(*diverse_sub_slot(st, t, threadIdx.x & 63));
}

__global__ void diverse_clear_kernel(unsigned long long* records, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) records[i] = 0ull;
}

// domain_grid_kernel's passes over the reference, with another last stage.  MXR = 32 or 64 as there.  Three waves a
// SIMD as there (168 registers): the last stage's few more would otherwise cost the third.
template <int MXR>
__global__ __launch_bounds__(256, 3) void diverse_init_kernel(const float* __restrict__ mix_cat,
                                                           const float* __restrict__ mix_an,
                                                           const float* __restrict__ ref,
                                                           const uint32_t* __restrict__ where, DiverseState st, int k,
                                                           int C, int A, int R, int Mx, int tiles_a, int W) {
  extern __shared__ __align__(16) float sm[];
  constexpr int P = kDomainRegs / MXR;
  const int S = mix_row_stride(Mx), S2 = (int)align4(Mx);
  float* man = sm;                  // [kTileA][S]
  float* mcat = man + kTileA * S;   // [kTileC][S]
  float* chunk = mcat + kTileC * S; // [kDomainChunk][S2]
  DiverseScratch* sc = reinterpret_cast<DiverseScratch*>(chunk + kDomainChunk * S2);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = (int)(blockIdx.x / tiles_a) * kTileC, a0 = (int)(blockIdx.x % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);
  const float nan = __uint_as_float(0x7FC00000u);

  if (where) {  // a tile without a set bit: no pair of it competes, before any row is loaded
    uint32_t word = 0;
    if (tid < kWhereTileWords) {
      const int r = tid >> 1, w = (a0 >> 5) + (tid & 1);
      if (r < nc && w < W) word = where[(int64_t)(c0 + r) * W + w];
      sc->words[tid] = word;
    }
    if (!__syncthreads_or(word != 0)) {
      for (int e = tid; e < kTilePairs; e += 256) {
        const int r = e >> 6, a = e & 63;
        if (r < nc && a < na) st.plane[(int64_t)(c0 + r) * A + a0 + a] = nan;
      }
      if (tid == 0) st.flags[blockIdx.x] = 1u;
      return;
    }
  }

  domain_stage(man, mix_an + (int64_t)a0 * Mx, na, Mx, S2, S);
  domain_stage(mcat, mix_cat + (int64_t)c0 * Mx, nc, Mx, S2, S);
  __syncthreads();

  const float* pa = man + min(lane, na - 1) * S;
  unsigned long long key = 0;
  uint32_t count = 0;  // wave-uniform
  for (int s = 0; s < 4 / P; ++s) {
    const int first = wave + 4 * s * P;
    const bool work = first < nc;  // wave-uniform
    float z[P][MXR], best[P];
    int nearest[P], self[P];
#pragma unroll
    for (int q = 0; q < P; ++q) best[q] = __uint_as_float(0x7F800000u), nearest[q] = -1, self[q] = -1;
    domain_latent<MXR, P>(z, mcat, pa, first, nc, Mx, S);
    for (int p0 = 0; p0 < R; p0 += kDomainChunk) {
      const int n = min(kDomainChunk, R - p0);
      __syncthreads();  // the last chunk's readers
      domain_stage(chunk, ref + (int64_t)p0 * Mx, n, Mx, S2, S2);
      __syncthreads();
      if (work) domain_scan<MXR, P, false>(z, chunk, n, p0, Mx, S2, self, best, nearest);
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int ci = first + 4 * q;
      const bool in_grid = ci < nc && lane < na;
      bool live = in_grid;
      if (where) live = live && ((sc->words[min(ci, kTileC - 1) * 2 + (lane >> 5)] >> (lane & 31)) & 1u);
      const float d = live ? domain_result(best[q], nearest[q]) : nan;
      const uint32_t pair = (uint32_t)(c0 + ci) * (uint32_t)A + (uint32_t)(a0 + lane);
      if (in_grid) st.plane[(int64_t)(c0 + ci) * A + a0 + lane] = d;
      const bool cand = live && d > 0.f;
      if (cand) {
        const unsigned long long mine = diverse_key(d, pair);
        key = mine > key ? mine : key;
      }
      count += (uint32_t)__popcll(__ballot(cand));
    }
  }
  if (lane == 0) sc->count[wave] = count;
  const bool any = diverse_offer(sc, key, diverse_sub_slot(st, 0, blockIdx.x % kDiverseSubSlots));  // (its barrier publishes the counts)
  if (tid == 0) {
    st.flags[blockIdx.x] = any ? 0u : 1u;
    const uint32_t total = sc->count[0] + sc->count[1] + sc->count[2] + sc->count[3];
    if (total) atomicAdd(st.records + (size_t)k * kDiverseSlotWords, (unsigned long long)total);
  }
}

__host__ __device__ inline size_t diverse_step_lds_bytes(int Mx) {
  return sizeof(float) * ((size_t)(kTileA + kTileC) * mix_row_stride(Mx) + align4(Mx) + kTilePairs) + sizeof(DiverseScratch);
}

// Launch t >= 1.  VEC: A is a multiple of 4, the plane moves 16 bytes per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void diverse_step_kernel(const float* __restrict__ mix_cat,
                                                           const float* __restrict__ mix_an, DiverseState st, int t,
                                                           int C, int A, int Mx, int tiles_a) {
  extern __shared__ __align__(16) float sm[];
  // the tile's flag and the lane's sub-slot of pick t - 1 in one round trip, before any load of rows or state
  const uint32_t flagged = st.flags[blockIdx.x];
  const unsigned long long prev = diverse_pick(st, t - 1);
  if (flagged) return;                           // no candidate in the tile
  if (prev == 0) return;                         // the selection has ended
  const int S = mix_row_stride(Mx), S2 = (int)align4(Mx);
  float* man = sm;                   // [kTileA][S]
  float* mcat = man + kTileA * S;    // [kTileC][S]
  float* zc = mcat + kTileC * S;     // [S2]: the chosen pair's latent vector
  float* tile = zc + S2;             // [kTileC][kTileA]: the plane's tile
  DiverseScratch* sc = reinterpret_cast<DiverseScratch*>(tile + kTilePairs);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = (int)(blockIdx.x / tiles_a) * kTileC, a0 = (int)(blockIdx.x % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);
  const float nan = __uint_as_float(0x7FC00000u);
  const uint32_t chosen = ~(uint32_t)prev;
  const int cs = (int)(chosen / (uint32_t)A), as = (int)(chosen % (uint32_t)A);

  domain_stage(man, mix_an + (int64_t)a0 * Mx, na, Mx, S2, S);
  domain_stage(mcat, mix_cat + (int64_t)c0 * Mx, nc, Mx, S2, S);
  if (tid < S2) zc[tid] = tid < Mx ? mix_cat[(int64_t)cs * Mx + tid] + mix_an[(int64_t)as * Mx + tid] : 0.f;  // the cation term first
  // thread -> (row, quad of anions) of the tile for the 16-byte form, (row, anion) x 4 for the other
  const int vr = tid >> 4, va = (tid & 15) * 4;
  const bool vin = vr < nc && va < na;  // (A % 4 == 0: a quad lies inside the grid or outside)
  const int64_t ve = (int64_t)(c0 + vr) * A + a0 + va;
  if constexpr (VEC) {
    f32x4_t v = {nan, nan, nan, nan};
    if (vin) v = ld4(st.plane + ve);
    *reinterpret_cast<f32x4_t*>(tile + vr * kTileA + va) = v;
  } else {
#pragma unroll
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + tid, r = e >> 6, a = e & 63;
      tile[e] = r < nc && a < na ? st.plane[(int64_t)(c0 + r) * A + a0 + a] : nan;
    }
  }
  __syncthreads();

  const float* pa = man + min(lane, na - 1) * S;
  const float* pc[4];
  float d2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) pc[q] = mcat + min(wave + 4 * q, nc - 1) * S, d2[q] = 0.f;
  for (int k4 = 0; k4 < Mx; k4 += 4) {  // d2 = 0; diff = z[k] - r[k]; d2 = fmaf(diff, diff, d2), k ascending (zero pads)
    const f32x4_t a = ld4(pa + k4), r = ld4(zc + k4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4_t z = ld4(pc[q] + k4) + a;  // AddTwoTensors, the cation term first
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float diff = z[u] - r[u];
        d2[q] = fmaf(diff, diff, d2[q]);
      }
    }
  }
  unsigned long long key = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ci = wave + 4 * q;
    const float old = tile[ci * kTileA + lane], d = sqrtf(d2[q]);
    const float now = d < old ? d : old;  // min(D, dist); a NaN state stays NaN
    tile[ci * kTileA + lane] = now;
    if (ci < nc && lane < na && now > 0.f) {
      const unsigned long long mine = diverse_key(now, (uint32_t)(c0 + ci) * (uint32_t)A + (uint32_t)(a0 + lane));
      key = mine > key ? mine : key;
    }
  }
  const bool any = diverse_offer(sc, key, diverse_sub_slot(st, t, blockIdx.x % kDiverseSubSlots));  // (its barrier publishes the tile)
  if (tid == 0 && !any) st.flags[blockIdx.x] = 1u;
  if constexpr (VEC) {
    if (vin) *reinterpret_cast<f32x4_t*>(st.plane + ve) = ld4(tile + vr * kTileA + va);
  } else {
#pragma unroll
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + tid, r = e >> 6, a = e & 63;
      if (r < nc && a < na) st.plane[(int64_t)(c0 + r) * A + a0 + a] = tile[e];
    }
  }
}

// The slots -> the outputs; a wave per step.  The picks are a prefix of the steps: launch t returns when step t - 1 has
// none.
__global__ __launch_bounds__(256) void diverse_decode_kernel(DiverseState st, int k, int A, int32_t* __restrict__ cation,
                                                             int32_t* __restrict__ anion, float* __restrict__ distance,
                                                             int64_t* __restrict__ counts) {
  const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);  // wave-uniform
  if (i >= k) return;
  const unsigned long long rec = diverse_pick(st, i), next = i + 1 < k ? diverse_pick(st, i + 1) : 0ull;
  if ((threadIdx.x & 63) != 0) return;
  const uint32_t pair = ~(uint32_t)rec;
  cation[i] = rec ? (int32_t)(pair / (uint32_t)A) : -1;
  anion[i] = rec ? (int32_t)(pair % (uint32_t)A) : -1;
  distance[i] = rec ? __uint_as_float((uint32_t)(rec >> 32)) : __uint_as_float(0x7FC00000u);
  if (rec && !next) counts[0] = i + 1;
  if (i == 0) {
    if (!rec) counts[0] = 0;
    counts[1] = (int64_t)st.records[(size_t)k * kDiverseSlotWords];
  }
}

size_t diverse_record_words(int k) { return (size_t)k * kDiverseSlotWords + 1; }

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

DiverseState diverse_carve(void* workspace, int C, int A, int k) {
  char* base = static_cast<char*>(workspace);
  const size_t plane = align16(sizeof(float) * (size_t)C * A), records = align16(sizeof(unsigned long long) * diverse_record_words(k));
  return DiverseState{reinterpret_cast<float*>(base), reinterpret_cast<unsigned long long*>(base + plane),
                      reinterpret_cast<uint32_t*>(base + plane + records)};
}

}  // namespace

size_t diverse_workspace_bytes(int C, int A, int k) {
  return align16(sizeof(float) * (size_t)C * A) + align16(sizeof(unsigned long long) * diverse_record_words(k)) +
         align16(sizeof(uint32_t) * (size_t)grid_tiles(0, C, A).count());
}

int launch_diverse_select(const DiverseCall& c) {
  const GridTiles tiles = grid_tiles(0, c.C, c.A);
  if (int rc = grid_tiles_fit("diverse_select", tiles)) return rc;
  const DiverseState st = diverse_carve(c.workspace, c.C, c.A, c.k);
  const unsigned groups = (unsigned)tiles.count();
  const size_t words = diverse_record_words(c.k);
  diverse_clear_kernel<<<(unsigned)((words + 255) / 256), 256, 0, c.stream>>>(st.records, words);
  if (int rc = check_launch("diverse_clear")) return rc;
  const size_t init_lds = sizeof(float) * domain_grid_lds_floats(c.Mx) + sizeof(DiverseScratch);
  auto init = [&](auto kern) {
    kern<<<groups, 256, init_lds, c.stream>>>(c.mix_cat, c.mix_an, c.ref, c.where, st, c.k, c.C, c.A, c.R, c.Mx, tiles.a,
                                              mask_row_words(c.A));
  };
  c.Mx <= 32 ? init(diverse_init_kernel<32>) : init(diverse_init_kernel<64>);
  if (int rc = check_launch("diverse_init")) return rc;
  const size_t step_lds = diverse_step_lds_bytes(c.Mx);  // at most 26 288 bytes
  const bool vec = (c.A & 3) == 0;
  for (int t = 1; t < c.k; ++t) {
    if (vec)
      diverse_step_kernel<true><<<groups, 256, step_lds, c.stream>>>(c.mix_cat, c.mix_an, st, t, c.C, c.A, c.Mx, tiles.a);
    else
      diverse_step_kernel<false><<<groups, 256, step_lds, c.stream>>>(c.mix_cat, c.mix_an, st, t, c.C, c.A, c.Mx, tiles.a);
  }
  if (int rc = check_launch("diverse_step")) return rc;
  diverse_decode_kernel<<<(unsigned)((c.k + 3) / 4), 256, 0, c.stream>>>(st, c.k, c.A, c.cation, c.anion, c.distance, c.counts);
  return check_launch("diverse_decode");
}

}  // namespace impnn
