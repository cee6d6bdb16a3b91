// Device code the grid kernels share: the tile bodies of head_grid.hip and transfer_grid.hip, which the materialising
// kernels (impnn_head_grid, impnn_transfer_head_grid), the selecting kernels (grid_select.hip: impnn_head_grid_topk,
// impnn_transfer_head_grid_topk and their _where forms) and the mask-writing kernels (grid_mask.hip:
// impnn_head_grid_mask, impnn_transfer_head_grid_mask) and the partner-selecting kernels (grid_partners.hip:
// impnn_head_grid_partners, impnn_transfer_head_grid_partners) and the rank-cut kernels (grid_rank.hip:
// impnn_head_grid_rank, impnn_transfer_head_grid_rank) and the per-ion summary kernels (grid_summary.hip:
// impnn_*_grid_summary) all run, and the keys and the running top-k of the selection.
// One definition of a tile's arithmetic, so a selected or tested value has the bits the materialised grid holds for
// that pair; and, at the end, the one host function that launches them (launch_grid_family).
#pragma once

#include "common.h"
#include "head_device.h"

namespace impnn {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x4_t ld4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }

__host__ __device__ inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// ================================================================ selection (grid_select.hip)
// An entry is (key << 32) | pair index.  The key is the order-preserving integer image of the float's bits (sign bit
// flipped for non-negatives, all bits flipped for negatives: -0.0 < +0.0), complemented for `largest`; any NaN has the
// key 0xFFFFFFFF in both directions, which no other value has (it would be the image of a NaN's bits).  Entries are
// unique, compared as unsigned 64-bit integers: the total order (value, cation index, anion index), NaN last.
constexpr unsigned long long kSelectNone = ~0ull;  // no entry: pair indices stay below 2^32 - 1

__device__ __forceinline__ uint32_t select_key(float v, bool largest) {
  const uint32_t u = __float_as_uint(v);
  const uint32_t key = (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
  return v != v ? 0xFFFFFFFFu : (largest ? ~key : key);
}

__device__ __forceinline__ float select_value(uint32_t key, bool largest) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);  // the canonical quiet NaN
  if (largest) key = ~key;
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// The running selection of one temperature, in LDS: buf[0 .. count) are the entries kept so far, in no order after
// the first `kept`; `bound` is the k-th smallest entry at the last compaction, or kSelectNone before k entries were
// seen.  An entry at or above the bound cannot be among the k smallest.
struct SelectList {
  unsigned long long* buf;    // [cap], cap a power of two >= k + the entries one round can offer
  unsigned long long* bound;  // [1]
  int* count;                 // [1]
};

// Sorts buf[0 .. count) ascending and keeps the first k: a bitonic network over the next power of two, the tail padded
// with kSelectNone.  Every thread of the workgroup calls it with the same arguments, between barriers of its own.
__device__ __forceinline__ int select_compact(const SelectList& s, int count, int k) {
  const int tid = threadIdx.x;
  int P = 2;
  while (P < count) P <<= 1;
  for (int i = count + tid; i < P; i += blockDim.x) s.buf[i] = kSelectNone;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (P >> 1); i += blockDim.x) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const unsigned long long a = s.buf[lo], b = s.buf[hi];
        if ((a > b) == ((lo & size) == 0)) s.buf[lo] = b, s.buf[hi] = a;
      }
      __syncthreads();
    }
  const int kept = min(count, k);
  if (tid == 0) {
    *s.count = kept;
    *s.bound = kept == k ? s.buf[k - 1] : kSelectNone;
  }
  __syncthreads();
  return kept;
}

// Before a round that offers at most `round` entries: compacts when the list could not take them, or as soon as k
// entries have been seen and there is no bound yet.  Block-uniform; the offers of the last round are behind a barrier.
__device__ __forceinline__ void select_make_room(const SelectList& s, int k, int cap, int round) {
  const int count = *s.count;
  const bool unbounded = *s.bound == kSelectNone;
  __syncthreads();  // (every thread has read count and bound before thread 0 of select_compact rewrites them)
  if (count + round > cap || (unbounded && count >= k)) select_compact(s, count, k);
}

// A wave offers one entry per lane (`live` lanes): the survivors of the bound are appended with one ballot, one
// popcount and one integer LDS atomic per wave.
__device__ __forceinline__ void select_offer(const SelectList& s, unsigned long long bound, bool live,
                                             unsigned long long entry) {
  const bool pass = live && entry < bound;
  const unsigned long long mask = __ballot(pass);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(s.count, __popcll(mask));
  base = __shfl(base, 0);
  if (pass) s.buf[base + __popcll(mask & ((1ull << lane) - 1))] = entry;
}

__host__ __device__ inline int select_capacity(int k, int round) {
  int cap = 2;
  while (cap < k + round) cap <<= 1;
  return cap;
}

// carves nT lists of `cap` entries from 8-byte aligned LDS at `base`; list t is out[t]
__device__ __forceinline__ SelectList select_list(void* base, int nT, int cap, int t) {
  unsigned long long* bufs = reinterpret_cast<unsigned long long*>(base);
  unsigned long long* bounds = bufs + (size_t)nT * cap;
  int* counts = reinterpret_cast<int*>(bounds + nT);
  return SelectList{bufs + (size_t)t * cap, bounds + t, counts + t};
}
__host__ __device__ inline size_t select_lds_bytes(int nT, int cap) { return (size_t)nT * ((size_t)cap * 8 + 8 + 8); }

// What a selecting launch adds to a grid kernel's arguments: the trailing pack of head_grid_kernel and
// transfer_grid_kernel.  With it a workgroup is persistent: it walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
// and, where the materialising form stores a tile, offers the tile's values to its lists; at the end it writes its k
// kept entries per temperature, sorted, to ws [gridDim.x][nT][k] (unused slots kSelectNone).
struct GridSelect {
  unsigned long long* ws;
  int k, cap, largest;
  unsigned tiles;
};

// (the barriers between a kernel's loads and its first select_tile publish the empty lists)
__device__ __forceinline__ void select_init(const GridSelect& g, float* lds, int nT) {
  if ((int)threadIdx.x < nT) {
    const SelectList s = select_list(lds, nT, g.cap, threadIdx.x);
    *s.count = 0;
    *s.bound = kSelectNone;
  }
}

// A tile's `round` values (a multiple of the 256 threads; behind a barrier) against the lists:
// value(q, t, &live, &pair) is thread tid's q-th value at temperature t, whether it is a pair of the grid, and its index.
template <class Fn>
__device__ __forceinline__ void select_tile(const GridSelect& g, float* lds, int nT, int round, Fn value) {
  for (int t = 0; t < nT; ++t) select_make_room(select_list(lds, nT, g.cap, t), g.k, g.cap, round);
  for (int q = 0; q < round / 256; ++q)
    for (int t = 0; t < nT; ++t) {
      bool live;
      uint32_t pair;
      const float v = value(q, t, &live, &pair);
      const SelectList s = select_list(lds, nT, g.cap, t);
      select_offer(s, *s.bound, live, ((unsigned long long)select_key(v, g.largest != 0) << 32) | pair);
    }
  __syncthreads();  // the tile's regions are free for the next tile, the offers are in the lists
}

__device__ __forceinline__ bool select_next_tile(unsigned*) { return false; }
__device__ __forceinline__ bool select_next_tile(unsigned* tile, const GridSelect& g) {
  *tile += gridDim.x;
  return *tile < g.tiles;
}

__device__ __forceinline__ void select_finish(const GridSelect& g, float* lds, int nT) {
  for (int t = 0; t < nT; ++t) {
    const SelectList s = select_list(lds, nT, g.cap, t);
    const int kept = select_compact(s, *s.count, g.k);
    unsigned long long* dst = g.ws + ((size_t)blockIdx.x * nT + t) * g.k;
    for (int i = threadIdx.x; i < g.k; i += blockDim.x) dst[i] = i < kept ? s.buf[i] : kSelectNone;
  }
}

// ================================================================ pair masks (grid_mask.hip; grid_select.hip)
// The packed pair mask of include/impnn.h: words[C][W], W = ceil(A / 32), pair (i, j) is bit j & 31 of
// words[i][j >> 5], pad bits 0.  Both tile shapes start a tile on a word boundary (64 and 32 anions), so a word
// belongs to one workgroup.
__host__ __device__ inline int mask_row_words(int A) { return (int)(((int64_t)A + 31) >> 5); }

// A selecting launch over a masked grid: GridSelect plus the mask.  Only pairs whose bit is set compete, and a
// workgroup passes over a tile none of whose bits is set before it loads a row.  The tile's words sit in LDS behind
// the lists ([kWhereTileWords]).
constexpr int kWhereTileWords = 32;  // the larger tile: 16 cations x 2 words
struct GridSelectWhere : GridSelect {
  const uint32_t* where;  // [C][W]
  int W;
};

// What a mask-writing launch adds: where the materialising form stores a tile, this one tests lo <= v && v <= hi (a NaN
// fails both), ballots, and one lane per 32-pair span writes the word.  A viscosity mask is [nT][C][W].
struct GridMask {
  uint32_t* words;
  float lo, hi;
  int W;
};

// What a partner-selecting launch adds (grid_partners.hip): where the materialising form stores a tile, this one selects
// from the tile's values in LDS the m first entries of every tile row (a cation's anions) and of every tile column (an
// anion's cations) under the selection's order, and writes them, ascending, to rows [nT][tiles_a][C][m] and cols
// [nT][tiles_c][A][m] (kSelectNone where a row or column has fewer).  One tile per workgroup and one writing workgroup
// per slot: no pre-zeroing, no atomics.
struct GridPartners {
  unsigned long long *rows, *cols;
  int m, largest;
};
// ... over a masked grid: only pairs whose bit is set compete.  The tile's words sit in LDS behind the tile's regions
// ([kWhereTileWords]); a tile without a set bit is passed over before a row is loaded, its slots written kSelectNone.
struct GridPartnersWhere : GridPartners {
  const uint32_t* where;  // [C][W]
  int W;
};

// What the rank cut adds (grid_rank.hip): the k-th entry of the selection's order by a most-significant-digit radix select
// over the 64-bit entries, kRankDigitBits bits a pass.  The state of one plane between the launches of a call, in the
// workspace: the digits found so far (the bits of `prefix` above the current digit), the rank that remains inside the
// entries that share them, and after the last pass the k-th entry itself, `bound` (kSelectNone, latched by `none`, when
// fewer than k pairs compete).
struct RankState {
  unsigned long long prefix, rank, bound;
  uint32_t count, none;
};
// The counting form.  With it a workgroup is persistent, as with GridSelect, and where the materialising form stores a
// tile it counts the tile's entries whose bits above `shift + kRankDigitBits` equal the plane's prefix by their digit
// at `shift`, into an LDS histogram [planes][kRankBins] behind the tile's regions (integer LDS atomics); at the end it
// writes all of its counters to hist [gridDim.x][planes][kRankBins].  `where` may be null: every pair competes.
struct GridRank {
  const RankState* state;  // [planes]; not read by the first pass (shift + kRankDigitBits == 64)
  uint32_t* hist;
  const uint32_t* where;   // [C][W], or null
  int W, shift, largest;
  unsigned tiles;
};
// The mask form: one tile per workgroup, as GridMask; the bit of a pair is in-grid && where bit && entry <= bound of
// its plane.  A viscosity mask is [nT][C][W].
struct GridMaskRank {
  uint32_t* words;
  const RankState* state;  // [planes]
  const uint32_t* where;   // [C][W], or null
  int W, largest;
};

// What the summary form adds (grid_summary.hip): where the materialising form stores a tile, this one reduces the tile's
// values along every tile row (a cation's anions of this tile) and every tile column (an anion's cations of this tile)
// to one record each and writes them to rows [planes][tiles_a][C] and cols [planes][tiles_c][A].  One tile per
// workgroup and one writing workgroup per slot: no pre-zeroing, no atomics.  A pair competes when its `where` bit is
// set (null: always) and its value is not NaN.  The record of the competing pairs: their number n, s = sum (double)v,
// q = sum (double)v * (double)v (the product of two float32 values is exact in double), and lo / hi, the least keys of
// select_key(v, false) / select_key(v, true), 0xFFFFFFFF where nothing competes.  The order of the sums is fixed: a tile
// row is the adjacent-pair tree x[2k] + x[2k+1], level by level, over the row's lanes, a lane that does not compete
// holding +0.0; a tile column starts at +0.0 and adds its rows in ascending order.
struct SummaryRecord {
  double s, q;
  uint32_t n, lo, hi, pad;
};
static_assert(sizeof(SummaryRecord) == 32, "a summary record is 32 bytes");
struct GridSummary {
  SummaryRecord *rows, *cols;
  const uint32_t* where;  // [C][W], or null
  int W;
};

// which form of a grid kernel its trailing pack makes
template <class... Sel> struct GridForm { static constexpr bool select = false, where = false, mask = false, partners = false, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridSelect> { static constexpr bool select = true, where = false, mask = false, partners = false, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridSelectWhere> { static constexpr bool select = true, where = true, mask = false, partners = false, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridMask> { static constexpr bool select = false, where = false, mask = true, partners = false, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridPartners> { static constexpr bool select = false, where = false, mask = false, partners = true, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridPartnersWhere> { static constexpr bool select = false, where = true, mask = false, partners = true, rank_count = false, rank_mask = false, summary = false; };
template <> struct GridForm<GridRank> { static constexpr bool select = false, where = false, mask = false, partners = false, rank_count = true, rank_mask = false, summary = false; };
template <> struct GridForm<GridSummary> { static constexpr bool select = false, where = false, mask = false, partners = false, rank_count = false, rank_mask = false, summary = true; };
template <> struct GridForm<GridMaskRank> { static constexpr bool select = false, where = false, mask = false, partners = false, rank_count = false, rank_mask = true, summary = false; };

__device__ __forceinline__ bool select_next_tile(unsigned*, const GridMask&) { return false; }
__device__ __forceinline__ bool select_next_tile(unsigned*, const GridPartners&) { return false; }
__device__ __forceinline__ bool select_next_tile(unsigned*, const GridMaskRank&) { return false; }
__device__ __forceinline__ bool select_next_tile(unsigned*, const GridSummary&) { return false; }
__device__ __forceinline__ bool select_next_tile(unsigned* tile, const GridRank& g) {
  *tile += gridDim.x;
  return *tile < g.tiles;
}

// the tile's mask words in LDS; `lists` is the LDS behind the tile's regions
__device__ __forceinline__ uint32_t* where_tile_words(const GridSelectWhere& g, float* lists, int nT) {
  return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lists) + select_lds_bytes(nT, g.cap));
}
__device__ __forceinline__ uint32_t* where_tile_words(const GridPartnersWhere&, float* lists, int) {
  return reinterpret_cast<uint32_t*>(lists);
}
__device__ __forceinline__ uint32_t* where_tile_words(const GridRank&, float* lists, int nT) {  // behind the histogram
  return reinterpret_cast<uint32_t*>(lists) + (size_t)nT * kRankBins;
}
__device__ __forceinline__ uint32_t* where_tile_words(const GridMaskRank&, float* lists, int) {
  return reinterpret_cast<uint32_t*>(lists);
}
__device__ __forceinline__ uint32_t* where_tile_words(const GridSummary&, float* lists, int) {
  return reinterpret_cast<uint32_t*>(lists);
}

// Loads the words of the tile's rows c0 .. c0 + nc, `wpr` words per row from anion word w0, into LDS (word r * wpr + w;
// 0 where the grid has no such word) and returns whether any bit is set.  Block-uniform: every thread of the workgroup
// calls it, and it is a barrier (the last tile's readers of these words are behind select_tile's).
template <class Where>
__device__ __forceinline__ bool where_tile_any(const Where& g, float* lists, int nT, int c0, int nc, int w0, int wpr) {
  const int tid = threadIdx.x;
  uint32_t word = 0;
  if (tid < kWhereTileWords) {
    const int r = tid / wpr, w = w0 + tid % wpr;
    if (r < nc && w < g.W) word = g.where[(int64_t)(c0 + r) * g.W + w];
    where_tile_words(g, lists, nT)[tid] = word;
  }
  return __syncthreads_or(word != 0) != 0;
}

// the bit of the tile's pair (row r, anion a of the tile), after where_tile_any
template <class Where>
__device__ __forceinline__ bool where_bit(const Where& g, float* lists, int nT, int r, int a, int wpr) {
  return (where_tile_words(g, lists, nT)[r * wpr + (a >> 5)] >> (a & 31)) & 1u;
}

// A wave's ballot of `pass` as the mask words of its 64 lanes: lane 0 writes the low word to lo_word, lane 32 the high
// word to hi_word (null: no such word in the grid).  Ordinary vector stores.
__device__ __forceinline__ void mask_store_ballot(bool pass, uint32_t* lo_word, uint32_t* hi_word) {
  const unsigned long long b = __ballot(pass);
  const int lane = threadIdx.x & 63;
  if (lane == 0 && lo_word) *lo_word = (uint32_t)b;
  if (lane == 32 && hi_word) *hi_word = (uint32_t)(b >> 32);
}

__device__ __forceinline__ uint32_t* mask_word(const GridMask& g, int64_t row, int w) { return g.words + (int64_t)row * g.W + w; }
__device__ __forceinline__ bool mask_passes(const GridMask& g, float v) { return g.lo <= v && v <= g.hi; }

// The head grid's tile as mask words: value(e, t) is pair e = r * kTileA + a of the tile at temperature t.  A wave's
// 64 lanes are the 64 anions of one tile row, i.e. that row's two words.
template <class Fn>
__device__ __forceinline__ void mask_head_tile(const GridMask& g, int C, int c0, int a0, int nc, int na, int nT, Fn value) {
  for (int t = 0; t < nT; ++t)
    for (int q = 0; q < 4; ++q) {  // kTilePairs / 256 threads
      const int e = q * 256 + (int)threadIdx.x, r = e >> 6, a = e & 63;
      const float v = value(e, t);
      uint32_t* row = mask_word(g, t * (int64_t)C + c0 + r, a0 >> 5);
      mask_store_ballot(r < nc && a < na && mask_passes(g, v), r < nc ? row : nullptr,
                        r < nc && (a0 >> 5) + 1 < g.W ? row + 1 : nullptr);
    }
}

// ================================================================ best partners (grid_partners.hip)
// The entry of a tile's pair, or kSelectNone for a lane that is no pair of the grid or whose mask bit is clear.
__device__ __forceinline__ unsigned long long partners_entry(const GridPartners& g, bool live, float v, uint32_t pair) {
  return live ? ((unsigned long long)select_key(v, g.largest != 0) << 32) | pair : kSelectNone;
}

// x of the lane a DPP control names (a permutation inside a row of 16 lanes; every lane of the wave is active)
template <int CTRL>
__device__ __forceinline__ unsigned long long partners_dpp(unsigned long long x) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(x >> 32), CTRL, 0xF, 0xF, false);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long partners_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// The unsigned 64-bit minimum over a row of WIDTH = 64 or 32 lanes, in every lane of the row: four DPP steps inside
// the 16-lane rows (lane ^ 1, lane ^ 2, the mirrors of 8 and 16), then lane ^ 16 (and lane ^ 32) by shuffle.
template <int WIDTH>
__device__ __forceinline__ unsigned long long partners_row_min(unsigned long long x) {
  x = partners_min(x, partners_dpp<0xB1>(x));   // quad_perm [1,0,3,2]
  x = partners_min(x, partners_dpp<0x4E>(x));   // quad_perm [2,3,0,1]
  x = partners_min(x, partners_dpp<0x141>(x));  // row_half_mirror
  x = partners_min(x, partners_dpp<0x140>(x));  // row_mirror
  x = partners_min(x, __shfl_xor(x, 16));
  if (WIDTH == 64) x = partners_min(x, __shfl_xor(x, 32));
  return x;
}

// A tile row, one entry per lane of a row of WIDTH lanes: m rounds of the minimum, the winner retires after each
// (entries are unique), lane i of the row keeps round i's and the first m lanes write dst[0 .. m) (null: the grid has
// no such row).  Wave-uniform control flow.
template <int WIDTH>
__device__ __forceinline__ void partners_row(const GridPartners& g, unsigned long long entry, unsigned long long* dst) {
  const int l = threadIdx.x & (WIDTH - 1);
  unsigned long long mine = kSelectNone;
  for (int i = 0; i < g.m; ++i) {
    const unsigned long long mn = partners_row_min<WIDTH>(entry);
    if (l == i) mine = mn;
    if (entry == mn) entry = kSelectNone;
  }
  if (dst && l < g.m) dst[l] = mine;
}

// A tile column, one thread: the kPartnersMaxM smallest entries offered so far, ascending, in registers (every index
// is a constant after unrolling).
struct PartnersBest {
  unsigned long long e[kPartnersMaxM];
  __device__ __forceinline__ PartnersBest() {
#pragma unroll
    for (int i = 0; i < kPartnersMaxM; ++i) e[i] = kSelectNone;
  }
  __device__ __forceinline__ void offer(unsigned long long cand) {
#pragma unroll
    for (int i = 0; i < kPartnersMaxM; ++i) {
      const unsigned long long b = e[i];
      const bool first = cand < b;
      e[i] = first ? cand : b;
      cand = first ? b : cand;
    }
  }
  __device__ __forceinline__ void store(unsigned long long* dst, int m) const {
#pragma unroll
    for (int i = 0; i < kPartnersMaxM; ++i)
      if (i < m) dst[i] = e[i];
  }
};

// The slots of a tile the mask lets the workgroup pass over: rows c0 .. c0 + nc of anion tile ta and columns a0 .. a0 + na
// of cation tile tc, every plane, all kSelectNone (each run of slots is contiguous).
__device__ __forceinline__ void partners_skip_tile(const GridPartners& g, int C, int A, int c0, int a0, int nc, int na,
                                                   int tiles_a, int ta, int tiles_c, int tc, int planes) {
  for (int t = 0; t < planes; ++t) {
    unsigned long long* rows = g.rows + (((size_t)t * tiles_a + ta) * C + c0) * g.m;
    unsigned long long* cols = g.cols + (((size_t)t * tiles_c + tc) * A + a0) * g.m;
    for (int i = threadIdx.x; i < nc * g.m; i += blockDim.x) rows[i] = kSelectNone;
    for (int i = threadIdx.x; i < na * g.m; i += blockDim.x) cols[i] = kSelectNone;
  }
}

// ================================================================ rank cut (grid_rank.hip)
__host__ __device__ inline size_t rank_lds_bytes(int planes) { return sizeof(uint32_t) * (size_t)planes * kRankBins; }

// whether the launch has a mask (block-uniform: a kernel argument)
__device__ __forceinline__ bool rank_masked(const GridRank& g) { return g.where != nullptr; }
__device__ __forceinline__ bool rank_masked(const GridMaskRank& g) { return g.where != nullptr; }

__device__ __forceinline__ unsigned long long rank_entry(float v, int largest, uint32_t pair) {
  return ((unsigned long long)select_key(v, largest != 0) << 32) | pair;
}

// (the barriers between a kernel's loads and its first rank_count publish the zeros)
__device__ __forceinline__ void rank_init(const GridRank&, float* lists, int planes) {
  uint32_t* hist = reinterpret_cast<uint32_t*>(lists);
  for (int i = threadIdx.x; i < planes * kRankBins; i += blockDim.x) hist[i] = 0;
}

// the plane's digits so far; the first pass has none and does not read the state
__device__ __forceinline__ unsigned long long rank_prefix(const GridRank& g, int t) {
  return g.shift + kRankDigitBits < 64 ? g.state[t].prefix : 0ull;
}

// A wave counts one entry per lane (`live` lanes) into hist[kRankBins] of its plane.  Entries of a tile crowd a few
// bins (the sign and exponent of the first pass; one bin per pass on a grid of equal values), so the wave's leading
// digit values are peeled first: the first pending lane's digit, a ballot of the lanes that share it, one atomic with
// their number; at most kRankPeel rounds, then one atomic per lane that is left.  Wave-uniform control flow.
constexpr int kRankPeel = 2;
__device__ __forceinline__ void rank_count(const GridRank& g, uint32_t* hist, unsigned long long prefix, bool live,
                                           unsigned long long entry) {
  const int hi = g.shift + kRankDigitBits;
  const bool match = live && (hi >= 64 || (entry >> hi) == (prefix >> hi));
  const uint32_t digit = (uint32_t)(entry >> g.shift) & (kRankBins - 1);
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(match);
  for (int round = 0; round < kRankPeel && todo != 0; ++round) {
    const int leader = __ffsll(todo) - 1;
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)digit, leader);
    const unsigned long long same = __ballot(match && digit == d);  // (a peeled lane has another digit)
    if (lane == leader) atomicAdd(hist + d, (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(hist + digit, 1u);
}

// all of the workgroup's counters, zeros included: every slot of hist has one writer and needs no zeroing
__device__ __forceinline__ void rank_finish(const GridRank& g, float* lists, int planes) {
  __syncthreads();
  const uint32_t* hist = reinterpret_cast<const uint32_t*>(lists);
  uint32_t* dst = g.hist + (size_t)blockIdx.x * planes * kRankBins;
  for (int i = threadIdx.x; i < planes * kRankBins; i += blockDim.x) dst[i] = hist[i];
}

// The words of a tile the mask lets the workgroup pass over (rows c0 .. c0 + nc, `wpr` words from word w0, every
// plane): the counting form owes nothing, the mask form is their only writer and writes them 0.
__device__ __forceinline__ void rank_skip_tile(const GridRank&, int, int, int, int, int, int) {}
__device__ __forceinline__ void rank_skip_tile(const GridMaskRank& g, int C, int c0, int nc, int w0, int wpr, int planes) {
  const int nw = min(wpr, g.W - w0);
  for (int i = threadIdx.x; i < planes * nc * nw; i += blockDim.x) {
    const int t = i / (nc * nw), r = (i / nw) % nc, w = i % nw;
    g.words[((int64_t)t * C + c0 + r) * g.W + w0 + w] = 0u;
  }
}

// ================================================================ per-ion summary (grid_summary.hip)
// whether the launch has a mask (block-uniform: a kernel argument)
__device__ __forceinline__ bool summary_masked(const GridSummary& g) { return g.where != nullptr; }

constexpr uint32_t kSummaryNoKey = 0xFFFFFFFFu;  // lo / hi of a record without a competing pair

// x + x of the lane a DPP control names: a double travels as its two halves (partners_dpp)
template <int CTRL>
__device__ __forceinline__ double summary_dpp_add(double x) {
  return x + __longlong_as_double((long long)partners_dpp<CTRL>((unsigned long long)__double_as_longlong(x)));
}
// The sum over a row of WIDTH = 64 or 32 lanes, in every lane of the row, by partners_row_min's butterfly.  Every step
// adds the two halves of a span that both hold their own sum, and a + b has the bits of b + a: the adjacent-pair tree
// x[2k] + x[2k+1], level by level, with the same bits in every lane.
template <int WIDTH>
__device__ __forceinline__ double summary_row_sum(double x) {
  x = summary_dpp_add<0xB1>(x);   // quad_perm [1,0,3,2]
  x = summary_dpp_add<0x4E>(x);   // quad_perm [2,3,0,1]
  x = summary_dpp_add<0x141>(x);  // row_half_mirror
  x = summary_dpp_add<0x140>(x);  // row_mirror
  x = x + __shfl_xor(x, 16);
  if (WIDTH == 64) x = x + __shfl_xor(x, 32);
  return x;
}
template <int CTRL>
__device__ __forceinline__ uint32_t summary_dpp_min(uint32_t x) {
  return min(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false));
}
template <int WIDTH>
__device__ __forceinline__ uint32_t summary_row_min(uint32_t x) {
  x = summary_dpp_min<0xB1>(x);
  x = summary_dpp_min<0x4E>(x);
  x = summary_dpp_min<0x141>(x);
  x = summary_dpp_min<0x140>(x);
  x = min(x, (uint32_t)__shfl_xor((int)x, 16));
  if (WIDTH == 64) x = min(x, (uint32_t)__shfl_xor((int)x, 32));
  return x;
}

// A tile row, one value per lane of a row of WIDTH lanes (`ok`: the lane's pair competes): the row's record, written by
// the row's first lane to dst (null: the grid has no such row).  Wave-uniform control flow, every lane active.
template <int WIDTH>
__device__ __forceinline__ void summary_row(bool ok, float v, SummaryRecord* dst) {
  const int lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(ok);
  const uint32_t n = WIDTH == 64 ? (uint32_t)__popcll(b) : (uint32_t)__popc((uint32_t)(b >> (lane & 32)));
  const double d = ok ? (double)v : 0.0;
  const double s = summary_row_sum<WIDTH>(d), q = summary_row_sum<WIDTH>(d * d);
  const uint32_t lo = summary_row_min<WIDTH>(ok ? select_key(v, false) : kSummaryNoKey);
  const uint32_t hi = summary_row_min<WIDTH>(ok ? select_key(v, true) : kSummaryNoKey);
  if (dst && (lane & (WIDTH - 1)) == 0) *dst = SummaryRecord{s, q, n, lo, hi, 0u};
}

// A record that grows one term, or one record, at a time in ascending order: a tile column (one thread walks the
// tile's rows) and the merge of an ion's partial records.  It starts as the record of no pair: n 0, sums +0.0, no keys.
struct SummarySum {
  double s = 0.0, q = 0.0;
  uint32_t n = 0u, lo = kSummaryNoKey, hi = kSummaryNoKey;
  __device__ __forceinline__ void add(bool ok, float v) {
    if (!ok) return;  // (s and q are never -0.0: adding the +0.0 of a pair that does not compete would change nothing)
    const double d = (double)v;
    s = s + d;
    q = q + d * d;
    n += 1u;
    lo = min(lo, select_key(v, false));
    hi = min(hi, select_key(v, true));
  }
  __device__ __forceinline__ void add(const SummaryRecord& r) {
    s = s + r.s;
    q = q + r.q;
    n += r.n;
    lo = min(lo, r.lo);
    hi = min(hi, r.hi);
  }
  __device__ __forceinline__ SummaryRecord record() const { return SummaryRecord{s, q, n, lo, hi, 0u}; }
};

// The slots of a tile the mask lets the workgroup pass over: rows c0 .. c0 + nc of anion tile ta and columns a0 .. a0 + na
// of cation tile tc, every plane, the record of no pair - what computing the tile would give.
__device__ __forceinline__ void summary_skip_tile(const GridSummary& g, int C, int A, int c0, int a0, int nc, int na,
                                                  int tiles_a, int ta, int tiles_c, int tc, int planes) {
  const SummaryRecord none = SummarySum().record();
  for (int t = 0; t < planes; ++t) {
    SummaryRecord* rows = g.rows + ((size_t)t * tiles_a + ta) * C + c0;
    SummaryRecord* cols = g.cols + ((size_t)t * tiles_c + tc) * A + a0;
    for (int i = threadIdx.x; i < nc; i += blockDim.x) rows[i] = none;
    for (int i = threadIdx.x; i < na; i += blockDim.x) cols[i] = none;
  }
}

// ================================================================ the head grid (head_grid.hip; grid_select.hip; grid_mask.hip; grid_partners.hip)
// One workgroup owns kTileC cations x kTileA anions; lane = anion, a wave walks the tile's cations.
constexpr int kTileC = 16, kTileA = 64, kTilePairs = kTileC * kTileA;

// Row stride (floats) of the mixing rows in LDS.  A lane reads its anion's row 16 bytes at a time (ds_read_b128: 16
// lanes per LDS cycle, 64 banks), so the 16 lanes of a group must start 4 banks apart: stride = 4 * odd.  Mx = 64
// unpadded would put all 64 lanes on one bank quad; the default Mx = 20 is 4 * 5 already.
__host__ __device__ inline int mix_row_stride(int Mx) {
  const int s = (Mx + 3) & ~3;
  return ((s >> 2) & 1) ? s : s + 4;
}

__host__ __device__ inline size_t grid_lds_floats(int kind, int nT, int F, int Mx) {
  const size_t rows = (size_t)(kTileA + kTileC) * mix_row_stride(Mx);
  if (kind == 0) return rows + align4((size_t)Mx * 3 + 3) + 3 * (size_t)kTilePairs + align4((size_t)nT);
  return rows + (size_t)F * align4(Mx) + align4(F) + align4((size_t)F + 1) + kTilePairs;
}


// The head grid's tile as partners: value(e, t) is pair e = r * kTileA + a of the tile at plane t, live(r, a) its mask
// bit.  A wave's 64 lanes are the 64 anions of one tile row; then one thread per (plane, tile column) walks the
// column's rows in LDS.
template <class Fn, class Live>
__device__ __forceinline__ void partners_head_tile(const GridPartners& g, int C, int A, int c0, int a0, int nc, int na,
                                                   int tiles_a, int planes, Fn value, Live live) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ta = a0 / kTileA, tc = c0 / kTileC, tiles_c = (C + kTileC - 1) / kTileC;
  for (int t = 0; t < planes; ++t)
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + tid, r = e >> 6;
      const bool ok = r < nc && lane < na && live(r, lane);
      const unsigned long long entry =
          partners_entry(g, ok, value(e, t), (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + lane));
      partners_row<kTileA>(g, entry, r < nc ? g.rows + (((size_t)t * tiles_a + ta) * C + c0 + r) * g.m : nullptr);
    }
  for (int item = tid; item < planes * kTileA; item += 256) {
    const int t = item >> 6, a = item & 63;
    if (a >= na) continue;
    PartnersBest best;
    for (int r = 0; r < nc; ++r)
      best.offer(partners_entry(g, live(r, a), value(r * kTileA + a, t), (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a)));
    best.store(g.cols + (((size_t)t * tiles_c + tc) * A + a0 + a) * g.m, g.m);
  }
}

// The head grid's tile as summary records: value(e, t) is pair e = r * kTileA + a of the tile at plane t, live(r, a) its
// mask bit.  A wave's 64 lanes are the 64 anions of one tile row; then one thread per (plane, tile column) walks the
// column's rows in LDS in ascending order.
template <class Fn, class Live>
__device__ __forceinline__ void summary_head_tile(const GridSummary& g, int C, int A, int c0, int a0, int nc, int na,
                                                  int tiles_a, int planes, Fn value, Live live) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int ta = a0 / kTileA, tc = c0 / kTileC, tiles_c = (C + kTileC - 1) / kTileC;
  for (int t = 0; t < planes; ++t)
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + tid, r = e >> 6;
      const float v = value(e, t);
      summary_row<kTileA>(r < nc && lane < na && live(r, lane) && v == v, v,
                          r < nc ? g.rows + ((size_t)t * tiles_a + ta) * C + c0 + r : nullptr);
    }
  for (int item = tid; item < planes * kTileA; item += 256) {
    const int t = item >> 6, a = item & 63;
    if (a >= na) continue;
    SummarySum sum;
    for (int r = 0; r < nc; ++r) {
      const float v = value(r * kTileA + a, t);
      sum.add(live(r, a) && v == v, v);
    }
    g.cols[((size_t)t * tiles_c + tc) * A + a0 + a] = sum.record();
  }
}

// The head grid's tile counted and as best-k mask words: value(e, t) is pair e = r * kTileA + a of the tile at plane t,
// live(r, a) its mask bit.  A wave's 64 lanes are the 64 anions of one tile row, i.e. that row's two words.
template <class Fn, class Live>
__device__ __forceinline__ void rank_head_tile(const GridRank& g, float* lists, int A, int c0, int a0, int nc, int na,
                                               int planes, Fn value, Live live) {
  uint32_t* hist = reinterpret_cast<uint32_t*>(lists);
  for (int t = 0; t < planes; ++t) {
    const unsigned long long prefix = rank_prefix(g, t);
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + (int)threadIdx.x, r = e >> 6, a = e & 63;
      const bool ok = r < nc && a < na && live(r, a);
      rank_count(g, hist + t * kRankBins, prefix, ok,
                 rank_entry(value(e, t), g.largest, (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a)));
    }
  }
  __syncthreads();  // the tile's regions and mask words are free for the next tile
}

template <class Fn, class Live>
__device__ __forceinline__ void rank_mask_head_tile(const GridMaskRank& g, int C, int A, int c0, int a0, int nc, int na,
                                                    int planes, Fn value, Live live) {
  for (int t = 0; t < planes; ++t) {
    const unsigned long long bound = g.state[t].bound;
    for (int q = 0; q < kTilePairs / 256; ++q) {
      const int e = q * 256 + (int)threadIdx.x, r = e >> 6, a = e & 63;
      const bool ok = r < nc && a < na && live(r, a);
      const unsigned long long entry = rank_entry(value(e, t), g.largest, (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a));
      uint32_t* row = g.words + ((int64_t)t * C + c0 + r) * g.W + (a0 >> 5);
      mask_store_ballot(ok && entry <= bound, r < nc ? row : nullptr, r < nc && (a0 >> 5) + 1 < g.W ? row + 1 : nullptr);
    }
  }
}

// Writes `rows` row spans of `span` floats each (row r starts at out + first + r * pitch) with 16-byte stores on
// every naturally aligned quad that lies inside the span and 4-byte stores on the ragged ends.  Element e of a span
// is value(r, e / per, e % per).  Consecutive threads take consecutive quads of a row: coalesced along the span.
template <class Fn>
__device__ __forceinline__ void store_rows(float* __restrict__ out, int64_t first, int64_t pitch, int rows, int span,
                                           int per, Fn value) {
  const int64_t po = (int64_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
  const int quads = (span + 3) / 4 + 1;  // quads a span can touch at any alignment
  for (int item = threadIdx.x; item < rows * quads; item += blockDim.x) {
    const int r = item / quads, q = item - r * quads;
    const int64_t g0 = first + (int64_t)r * pitch;
    const int e0 = 4 * q - (int)((g0 + po) & 3);  // out + g0 + e0 is 16-byte aligned
    if (e0 >= span) continue;
    const int e = e0 < 0 ? 0 : e0;
    int a = e / per, t = e - a * per;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = 0.f;
      if (e0 + u >= 0 && e0 + u < span) {
        v[u] = value(r, a, t);
        if (++t == per) t = 0, ++a;
      }
    }
    float* p = out + g0 + e0;
    if (e0 >= 0 && e0 + 3 < span) {
      // written once and not read again by the launch: a streaming (nontemporal) global_store_dwordx4
      __builtin_nontemporal_store(f32x4_t{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4_t*>(p));
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u >= 0 && e0 + u < span) p[u] = v[u];
    }
  }
}

// A pair of the tile as ensemble_grid_kernel evaluates it: head_grid_kernel's statements, restated (its own stay inline:
// its instantiations are kept instruction-identical to what they were before the ensemble grid existed).
// Kind 0: mixed = cation row + anion row (AddTwoTensors, the cation term first), vp = Dense(3) (bias first, inputs
// ascending), then the VFT parameters.  wts: Wv Mx*3 | bv 3.
__device__ __forceinline__ VftParams head_pair_vft(const float* cat_row, const float* an_row, const float* wts, int Mx) {
  const float4* pc = reinterpret_cast<const float4*>(cat_row);
  const float4* pa = reinterpret_cast<const float4*>(an_row);
  float v0 = wts[Mx * 3], v1 = wts[Mx * 3 + 1], v2 = wts[Mx * 3 + 2];
  for (int k4 = 0; k4 < Mx; k4 += 4) {
    const float4 c = pc[k4 >> 2], a = pa[k4 >> 2];
    const float m[4] = {c.x + a.x, c.y + a.y, c.z + a.z, c.w + a.w};  // AddTwoTensors, the cation term first
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k4 + u < Mx) {
        const float* w = wts + (k4 + u) * 3;
        v0 = fmaf(m[u], w[0], v0);
        v1 = fmaf(m[u], w[1], v1);
        v2 = fmaf(m[u], w[2], v2);
      }
  }
  return head_vft_params(v0, v1, v2);
}

// Kind 1: MXR registers hold the mixed vector, then relu(Dense(F)) and Dense(1).  whT [F][S2], bh [F], wo: Wo F | bo 1.
template <int MXR>
__device__ __forceinline__ float head_pair_mp(const float* cat_row, const float* an_row, const float* whT, const float* bh,
                                              const float* wo, int F, int Mx, int S2) {
  const float4* pc = reinterpret_cast<const float4*>(cat_row);
  const float4* pa = reinterpret_cast<const float4*>(an_row);
  float mixed[MXR];
#pragma unroll
  for (int k4 = 0; k4 < MXR; k4 += 4)
    if (k4 < Mx) {
      const float4 c = pc[k4 >> 2], a = pa[k4 >> 2];
      mixed[k4] = c.x + a.x, mixed[k4 + 1] = c.y + a.y, mixed[k4 + 2] = c.z + a.z, mixed[k4 + 3] = c.w + a.w;
    }
  float acc2 = wo[F];
  for (int j = 0; j < F; ++j) {
    const float4* w = reinterpret_cast<const float4*>(whT + j * S2);
    float acc = bh[j];
#pragma unroll
    for (int k4 = 0; k4 < MXR; k4 += 4)
      if (k4 < Mx) {
        const float4 ww = w[k4 >> 2];
        acc = fmaf(mixed[k4], ww.x, acc);
        if (k4 + 1 < Mx) acc = fmaf(mixed[k4 + 1], ww.y, acc);
        if (k4 + 2 < Mx) acc = fmaf(mixed[k4 + 2], ww.z, acc);
        if (k4 + 3 < Mx) acc = fmaf(mixed[k4 + 3], ww.w, acc);
      }
    acc2 = fmaf(head_relu(acc), wo[j], acc2);
  }
  return acc2;
}

// KIND 0: MXR unused (0).  KIND 1: MXR = 32 or 64 registers hold a pair's mixed vector.
template <int KIND, int MXR, class... Sel>
__global__ __launch_bounds__(256) void head_grid_kernel(const float* __restrict__ mix_cat,
                                                        const float* __restrict__ mix_an,
                                                        const float* __restrict__ T, const float* __restrict__ tail,
                                                        float* __restrict__ out, float* __restrict__ params, int C,
                                                        int A, int nT, int F, int Mx, int tiles_a, Sel... sel) {
  extern __shared__ __align__(16) float sm[];
  const int S = mix_row_stride(Mx);
  float* man = sm;                     // [kTileA][S]
  float* mcat = man + kTileA * S;      // [kTileC][S]
  float* wts = mcat + kTileC * S;      // the tail weights
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  using Form = GridForm<Sel...>;
  constexpr bool kSelect = Form::select;
  unsigned tile = blockIdx.x;
  if constexpr (kSelect) select_init(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1);
  if constexpr (Form::rank_count) rank_init(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1);
  do {
  const int c0 = (tile / tiles_a) * kTileC, a0 = (tile % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);
  if constexpr (Form::where) {  // a tile without a set bit: on to the next one, before any load
    if (!where_tile_any(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1, c0, nc, a0 >> 5, kTileA / 32)) {
      if constexpr (Form::partners)  // (its slots have no other writer)
        partners_skip_tile(sel..., C, A, c0, a0, nc, na, tiles_a, a0 / kTileA, (C + kTileC - 1) / kTileC, c0 / kTileC,
                           KIND == 0 ? nT : 1);
      continue;
    }
  }
  if constexpr (Form::rank_count || Form::rank_mask) {  // the rank forms' mask may be null: the same pass, when there is one
    if (rank_masked(sel...) &&
        !where_tile_any(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1, c0, nc, a0 >> 5, kTileA / 32)) {
      rank_skip_tile(sel..., C, c0, nc, a0 >> 5, kTileA / 32, KIND == 0 ? nT : 1);  // (its words have no other writer)
      continue;
    }
  }
  if constexpr (Form::summary) {  // the summary form's mask may be null too
    if (summary_masked(sel...) &&
        !where_tile_any(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1, c0, nc, a0 >> 5, kTileA / 32)) {
      summary_skip_tile(sel..., C, A, c0, a0, nc, na, tiles_a, a0 / kTileA, (C + kTileC - 1) / kTileC, c0 / kTileC,
                        KIND == 0 ? nT : 1);  // (its slots have no other writer)
      continue;
    }
  }

  // the tile's mixing rows: contiguous in global memory, padded rows in LDS (the pads are never used)
  for (int idx = tid; idx < na * Mx; idx += blockDim.x) {
    const int r = idx / Mx;
    man[r * S + (idx - r * Mx)] = mix_an[(int64_t)a0 * Mx + idx];
  }
  for (int idx = tid; idx < nc * Mx; idx += blockDim.x) {
    const int r = idx / Mx;
    mcat[r * S + (idx - r * Mx)] = mix_cat[(int64_t)c0 * Mx + idx];
  }

  if constexpr (KIND == 0) {
    const int nw = Mx * 3 + 3;         // Wv Mx*3 | bv 3
    float* resA = wts + ((nw + 3) & ~3);
    float* resB = resA + kTilePairs;
    float* resC = resB + kTilePairs;
    float* t100 = resC + kTilePairs;   // [nT]
    for (int t = tid; t < nw; t += blockDim.x) wts[t] = tail[t];
    for (int t = tid; t < nT; t += blockDim.x) t100[t] = head_scaled_t(T[t]);
    __syncthreads();
    for (int ci = wave; ci < nc; ci += 4) {
      if (lane < na) {
        const float4* pc = reinterpret_cast<const float4*>(mcat + ci * S);
        const float4* pa = reinterpret_cast<const float4*>(man + lane * S);
        float v0 = wts[Mx * 3], v1 = wts[Mx * 3 + 1], v2 = wts[Mx * 3 + 2];
        for (int k4 = 0; k4 < Mx; k4 += 4) {
          const float4 c = pc[k4 >> 2], a = pa[k4 >> 2];
          const float m[4] = {c.x + a.x, c.y + a.y, c.z + a.z, c.w + a.w};  // AddTwoTensors, the cation term first
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (k4 + u < Mx) {
              const float* w = wts + (k4 + u) * 3;
              v0 = fmaf(m[u], w[0], v0);
              v1 = fmaf(m[u], w[1], v1);
              v2 = fmaf(m[u], w[2], v2);
            }
        }
        const VftParams p = head_vft_params(v0, v1, v2);
        resA[ci * kTileA + lane] = p.A;
        resB[ci * kTileA + lane] = p.Bc;
        resC[ci * kTileA + lane] = p.Cc;
      }
    }
    __syncthreads();
    if constexpr (kSelect) {
      select_tile(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, kTilePairs, [&](int q, int t, bool* live, uint32_t* pair) {
        const int e = q * 256 + tid, r = e >> 6, a = e & 63;
        *live = r < nc && a < na;
        if constexpr (Form::where) *live = *live && where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, r, a, kTileA / 32);
        *pair = (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a);
        return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]);
      });
    } else if constexpr (Form::mask) {
      mask_head_tile(sel..., C, c0, a0, nc, na, nT, [&](int e, int t) {
        return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]);
      });
    } else if constexpr (Form::partners) {
      partners_head_tile(sel..., C, A, c0, a0, nc, na, tiles_a, nT,
                         [&](int e, int t) { return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]); },
                         [&](int r, int a) {
                           if constexpr (Form::where) return where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, r, a, kTileA / 32);
                           return true;
                         });
    } else if constexpr (Form::rank_count) {
      rank_head_tile(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), A, c0, a0, nc, na, nT,
                     [&](int e, int t) { return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]); },
                     [&](int r, int a) {
                       return !rank_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, r, a, kTileA / 32);
                     });
    } else if constexpr (Form::rank_mask) {
      rank_mask_head_tile(sel..., C, A, c0, a0, nc, na, nT,
                          [&](int e, int t) { return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]); },
                          [&](int r, int a) {
                            return !rank_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, r, a, kTileA / 32);
                          });
    } else if constexpr (Form::summary) {
      summary_head_tile(sel..., C, A, c0, a0, nc, na, tiles_a, nT,
                        [&](int e, int t) { return head_vft_eval(VftParams{resA[e], resB[e], resC[e]}, t100[t]); },
                        [&](int r, int a) {
                          return !summary_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), nT, r, a, kTileA / 32);
                        });
    } else {
    store_rows(out, ((int64_t)c0 * A + a0) * nT, (int64_t)A * nT, nc, na * nT, nT, [&](int r, int a, int t) {
      return head_vft_eval(VftParams{resA[r * kTileA + a], resB[r * kTileA + a], resC[r * kTileA + a]}, t100[t]);
    });
    if (params)
      store_rows(params, ((int64_t)c0 * A + a0) * 3, (int64_t)A * 3, nc, na * 3, 3, [&](int r, int a, int t) {
        return (t == 0 ? resA : t == 1 ? resB : resC)[r * kTileA + a];
      });
    }
  } else {
    const int S2 = (Mx + 3) & ~3;
    float* whT = wts;                         // [F][S2]: Wh transposed, a hidden unit's kernel column contiguous
    float* bh = whT + F * S2;                 // [F]
    float* wo = bh + ((F + 3) & ~3);          // Wo F | bo 1
    float* res = wo + ((F + 4) & ~3);         // [kTilePairs]
    for (int idx = tid; idx < Mx * F; idx += blockDim.x) {
      const int i = idx / F;
      whT[(idx - i * F) * S2 + i] = tail[idx];
    }
    for (int t = tid; t < F; t += blockDim.x) bh[t] = tail[Mx * F + t];
    for (int t = tid; t < F + 1; t += blockDim.x) wo[t] = tail[Mx * F + F + t];
    __syncthreads();
    for (int ci = wave; ci < nc; ci += 4) {
      if (lane < na) {
        const float4* pc = reinterpret_cast<const float4*>(mcat + ci * S);
        const float4* pa = reinterpret_cast<const float4*>(man + lane * S);
        float mixed[MXR];
#pragma unroll
        for (int k4 = 0; k4 < MXR; k4 += 4)
          if (k4 < Mx) {
            const float4 c = pc[k4 >> 2], a = pa[k4 >> 2];
            mixed[k4] = c.x + a.x, mixed[k4 + 1] = c.y + a.y, mixed[k4 + 2] = c.z + a.z, mixed[k4 + 3] = c.w + a.w;
          }
        float acc2 = wo[F];
        for (int j = 0; j < F; ++j) {
          const float4* w = reinterpret_cast<const float4*>(whT + j * S2);
          float acc = bh[j];
#pragma unroll
          for (int k4 = 0; k4 < MXR; k4 += 4)
            if (k4 < Mx) {
              const float4 ww = w[k4 >> 2];
              acc = fmaf(mixed[k4], ww.x, acc);
              if (k4 + 1 < Mx) acc = fmaf(mixed[k4 + 1], ww.y, acc);
              if (k4 + 2 < Mx) acc = fmaf(mixed[k4 + 2], ww.z, acc);
              if (k4 + 3 < Mx) acc = fmaf(mixed[k4 + 3], ww.w, acc);
            }
          acc2 = fmaf(head_relu(acc), wo[j], acc2);
        }
        res[ci * kTileA + lane] = acc2;
      }
    }
    __syncthreads();
    if constexpr (kSelect) {
      select_tile(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, kTilePairs, [&](int q, int, bool* live, uint32_t* pair) {
        const int e = q * 256 + tid, r = e >> 6, a = e & 63;
        *live = r < nc && a < na;
        if constexpr (Form::where) *live = *live && where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, r, a, kTileA / 32);
        *pair = (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a);
        return res[e];
      });
    } else if constexpr (Form::mask) {
      mask_head_tile(sel..., C, c0, a0, nc, na, 1, [&](int e, int) { return res[e]; });
    } else if constexpr (Form::partners) {
      partners_head_tile(sel..., C, A, c0, a0, nc, na, tiles_a, 1, [&](int e, int) { return res[e]; }, [&](int r, int a) {
        if constexpr (Form::where) return where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, r, a, kTileA / 32);
        return true;
      });
    } else if constexpr (Form::rank_count) {
      rank_head_tile(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), A, c0, a0, nc, na, 1, [&](int e, int) { return res[e]; },
                     [&](int r, int a) {
                       return !rank_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, r, a, kTileA / 32);
                     });
    } else if constexpr (Form::rank_mask) {
      rank_mask_head_tile(sel..., C, A, c0, a0, nc, na, 1, [&](int e, int) { return res[e]; }, [&](int r, int a) {
        return !rank_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, r, a, kTileA / 32);
      });
    } else if constexpr (Form::summary) {
      summary_head_tile(sel..., C, A, c0, a0, nc, na, tiles_a, 1, [&](int e, int) { return res[e]; }, [&](int r, int a) {
        return !summary_masked(sel...) || where_bit(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), 1, r, a, kTileA / 32);
      });
    } else {
    store_rows(out, (int64_t)c0 * A + a0, (int64_t)A, nc, na, 1, [&](int r, int a, int) { return res[r * kTileA + a]; });
    }
  }
  } while (select_next_tile(&tile, sel...));  // (the materialising form: one tile per workgroup)
  if constexpr (kSelect) select_finish(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1);
  if constexpr (Form::rank_count) rank_finish(sel..., sm + grid_lds_floats(KIND, nT, F, Mx), KIND == 0 ? nT : 1);
}

// ================================================================ the ensemble grid (ensemble_grid.hip)
// M members of one kind over the same tile: the statistic of a pair's M head values, one float per (pair, temperature)
// for the forms the head grid has - store, mask, top-k.  A member's value has the bits head_grid_kernel gives it for the
// same mixing rows (head_pair_vft / head_pair_mp, head_vft_eval); the statistic, in float32 and in this order:
//   s = v_0; s = s + v_m (m ascending); mean = s / M
//   q = 0; d = v_m - mean; q = fmaf(d, d, q) (m ascending); std = sqrt(q / M)      (the population deviation)
//   score = fmaf(kappa, std, mean)
// with the correctly rounded division and square root.  A NaN member value makes all three NaN, for that element only.
constexpr int kEnsembleMaxMembers = 8;
constexpr size_t kEnsembleLdsCap = 160 * 1024 - 256;  // a CU's LDS less the 256 static bytes of the _where form (__syncthreads_or)

struct EnsembleStat {
  float mean, std, score;
};
__device__ __forceinline__ EnsembleStat ensemble_stat(const float (&v)[kEnsembleMaxMembers], int M, float kappa) {
  float s = v[0];
#pragma unroll
  for (int m = 1; m < kEnsembleMaxMembers; ++m)
    if (m < M) s = s + v[m];
  const float n = (float)M, mean = s / n;
  float q = 0.f;
#pragma unroll
  for (int m = 0; m < kEnsembleMaxMembers; ++m)
    if (m < M) {
      const float d = v[m] - mean;
      q = fmaf(d, d, q);
    }
  const float sd = sqrtf(q / n);
  return EnsembleStat{mean, sd, fmaf(kappa, sd, mean)};
}

// the tail section of impnn_model_head's packed layout: kind 0 Wv Mx*3 | bv 3; kind 1 Wh Mx*F | bh F | Wo F | bo 1
__host__ __device__ inline size_t ensemble_tail_floats(int kind, int F, int Mx) {
  return kind == 0 ? (size_t)Mx * 3 + 3 : (size_t)Mx * F + 2 * (size_t)F + 1;
}
// The head grid's regions with M copies of the kept results (kind 0: a pair's three VFT parameters, kind 1: its value):
// 12 KiB and 4 KiB a member.  The mixing rows and the tail weights are one member's, loaded in turn.
__host__ __device__ inline size_t ensemble_lds_floats(int kind, int M, int nT, int F, int Mx) {
  return grid_lds_floats(kind, nT, F, Mx) + (size_t)(M - 1) * (kind == 0 ? 3 : 1) * kTilePairs;
}
// Temperatures one launch takes with M members at the widest rows the head kernels cover (kHeadMaxDim), so that the
// workgroup stays within kEnsembleLdsCap: a materialising or mask-writing launch (T / 100 sits in LDS, at most `most`),
// and a selecting launch (a list of select_capacity(kSelectMaxK, kTilePairs) entries per temperature and the tile's
// mask words behind the tile's regions; at most kSelectMaxT, and at least 1 for every M <= kEnsembleMaxMembers).
inline int ensemble_max_temperatures(int M, int most) {
  const size_t fixed = sizeof(float) * ensemble_lds_floats(0, M, 0, kHeadMaxDim, kHeadMaxDim);
  const size_t room = (kEnsembleLdsCap - fixed) / sizeof(float) & ~(size_t)3;
  return room < (size_t)most ? (int)room : most;
}
// ... and a summary launch: the tile's mask words sit behind the tile's regions (at most `most`)
inline int ensemble_summary_max_temperatures(int M, int most) {
  const size_t fixed = sizeof(float) * ensemble_lds_floats(0, M, 0, kHeadMaxDim, kHeadMaxDim) + sizeof(uint32_t) * kWhereTileWords;
  const size_t room = (kEnsembleLdsCap - fixed) / sizeof(float) & ~(size_t)3;
  return room < (size_t)most ? (int)room : most;
}
inline int ensemble_select_max_temperatures(int M) {
  int nT = kSelectMaxT;
  while (nT > 1 && sizeof(float) * ensemble_lds_floats(0, M, nT, kHeadMaxDim, kHeadMaxDim) +
                           select_lds_bytes(nT, select_capacity(kSelectMaxK, kTilePairs)) +
                           sizeof(uint32_t) * kWhereTileWords > kEnsembleLdsCap)
    --nT;
  return nT;
}

// What the materialising form writes: any of the three, (C,A,nT) for kind 0 and (C,A) for kind 1; a null one is skipped.
struct EnsembleOut {
  float *mean, *std, *score;
};

// mix_cat (M,C,Mx), mix_an (M,A,Mx), tails (M, ensemble_tail_floats).  The tile, its threads and its forms are
// head_grid_kernel's (store, GridMask, GridSelect, GridSelectWhere, GridSummary); the mask, the selection and the summary
// use the score.
template <int KIND, int MXR, class... Sel>
__global__ __launch_bounds__(256) void ensemble_grid_kernel(const float* __restrict__ mix_cat,
                                                            const float* __restrict__ mix_an,
                                                            const float* __restrict__ T, const float* __restrict__ tails,
                                                            EnsembleOut out, int M, float kappa, int C, int A, int nT,
                                                            int F, int Mx, int tiles_a, Sel... sel) {
  extern __shared__ __align__(16) float sm[];
  using Form = GridForm<Sel...>;
  static_assert(!Form::partners && !Form::rank_count && !Form::rank_mask, "ensemble grids: partners / rank are not built");
  constexpr bool kSelect = Form::select;
  constexpr int kKeep = KIND == 0 ? 3 : 1;  // floats kept per pair and member
  const int S = mix_row_stride(Mx), S2 = (Mx + 3) & ~3;
  float* man = sm;                     // [kTileA][S]
  float* mcat = man + kTileA * S;      // [kTileC][S]
  float* wts = mcat + kTileC * S;      // one member's tail weights, as head_grid_kernel lays them out
  float* kept = wts + (KIND == 0 ? align4((size_t)Mx * 3 + 3) : (size_t)F * S2 + align4(F) + align4((size_t)F + 1));
  float* t100 = kept + (size_t)M * kKeep * kTilePairs;  // [nT] (kind 0)
  float* lists = sm + ensemble_lds_floats(KIND, M, nT, F, Mx);
  const int planes = KIND == 0 ? nT : 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t ntail = ensemble_tail_floats(KIND, F, Mx);
  unsigned tile = blockIdx.x;
  if constexpr (kSelect) select_init(sel..., lists, planes);
  if constexpr (KIND == 0)
    for (int t = tid; t < nT; t += blockDim.x) t100[t] = head_scaled_t(T[t]);  // (published by the members' barriers)
  do {
  const int c0 = (tile / tiles_a) * kTileC, a0 = (tile % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);
  if constexpr (Form::where) {  // a tile without a set bit: on to the next one, before any load
    if (!where_tile_any(sel..., lists, planes, c0, nc, a0 >> 5, kTileA / 32)) continue;
  }
  if constexpr (Form::summary) {  // the summary form's mask may be null: the same pass, when there is one
    if (summary_masked(sel...) && !where_tile_any(sel..., lists, planes, c0, nc, a0 >> 5, kTileA / 32)) {
      summary_skip_tile(sel..., C, A, c0, a0, nc, na, tiles_a, a0 / kTileA, (C + kTileC - 1) / kTileC, c0 / kTileC, planes);
      continue;
    }
  }

  for (int m = 0; m < M; ++m) {
    if (m > 0) __syncthreads();  // the last member's pairs are done with the rows and the weights
    const float* rows_an = mix_an + ((int64_t)m * A + a0) * Mx;
    const float* rows_cat = mix_cat + ((int64_t)m * C + c0) * Mx;
    const float* tail = tails + (size_t)m * ntail;
    float* keep = kept + (size_t)m * kKeep * kTilePairs;
    for (int idx = tid; idx < na * Mx; idx += blockDim.x) {
      const int r = idx / Mx;
      man[r * S + (idx - r * Mx)] = rows_an[idx];
    }
    for (int idx = tid; idx < nc * Mx; idx += blockDim.x) {
      const int r = idx / Mx;
      mcat[r * S + (idx - r * Mx)] = rows_cat[idx];
    }
    if constexpr (KIND == 0) {
      for (int t = tid; t < Mx * 3 + 3; t += blockDim.x) wts[t] = tail[t];
      __syncthreads();
      for (int ci = wave; ci < nc; ci += 4)
        if (lane < na) {
          const VftParams p = head_pair_vft(mcat + ci * S, man + lane * S, wts, Mx);
          keep[ci * kTileA + lane] = p.A;
          keep[kTilePairs + ci * kTileA + lane] = p.Bc;
          keep[2 * kTilePairs + ci * kTileA + lane] = p.Cc;
        }
    } else {
      float* whT = wts;                   // [F][S2]
      float* bh = whT + F * S2;           // [F]
      float* wo = bh + ((F + 3) & ~3);    // Wo F | bo 1
      for (int idx = tid; idx < Mx * F; idx += blockDim.x) {
        const int i = idx / F;
        whT[(idx - i * F) * S2 + i] = tail[idx];
      }
      for (int t = tid; t < F; t += blockDim.x) bh[t] = tail[Mx * F + t];
      for (int t = tid; t < F + 1; t += blockDim.x) wo[t] = tail[Mx * F + F + t];
      __syncthreads();
      for (int ci = wave; ci < nc; ci += 4)
        if (lane < na) keep[ci * kTileA + lane] = head_pair_mp<MXR>(mcat + ci * S, man + lane * S, whT, bh, wo, F, Mx, S2);
    }
  }
  __syncthreads();

  // the statistic of pair e of the tile at temperature t, from the kept results (a pair outside the grid: unspecified
  // finite-or-not bits of stale LDS, never stored, never live)
  auto stat = [&](int e, int t) {
    float v[kEnsembleMaxMembers];
#pragma unroll
    for (int m = 0; m < kEnsembleMaxMembers; ++m) {
      v[m] = 0.f;
      if (m < M) {
        const float* keep = kept + (size_t)m * kKeep * kTilePairs + e;
        if constexpr (KIND == 0)
          v[m] = head_vft_eval(VftParams{keep[0], keep[kTilePairs], keep[2 * kTilePairs]}, t100[t]);
        else
          v[m] = keep[0];
      }
    }
    return ensemble_stat(v, M, kappa);
  };
  if constexpr (kSelect) {
    select_tile(sel..., lists, planes, kTilePairs, [&](int q, int t, bool* live, uint32_t* pair) {
      const int e = q * 256 + tid, r = e >> 6, a = e & 63;
      *live = r < nc && a < na;
      if constexpr (Form::where) *live = *live && where_bit(sel..., lists, planes, r, a, kTileA / 32);
      *pair = (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + a);
      return stat(e, t).score;
    });
  } else if constexpr (Form::mask) {
    mask_head_tile(sel..., C, c0, a0, nc, na, planes, [&](int e, int t) { return stat(e, t).score; });
  } else if constexpr (Form::summary) {
    summary_head_tile(sel..., C, A, c0, a0, nc, na, tiles_a, planes, [&](int e, int t) { return stat(e, t).score; },
                      [&](int r, int a) { return !summary_masked(sel...) || where_bit(sel..., lists, planes, r, a, kTileA / 32); });
  } else {
    const int64_t first = ((int64_t)c0 * A + a0) * planes, pitch = (int64_t)A * planes;
    if (out.mean)
      store_rows(out.mean, first, pitch, nc, na * planes, planes, [&](int r, int a, int t) { return stat(r * kTileA + a, t).mean; });
    if (out.std)
      store_rows(out.std, first, pitch, nc, na * planes, planes, [&](int r, int a, int t) { return stat(r * kTileA + a, t).std; });
    if (out.score)
      store_rows(out.score, first, pitch, nc, na * planes, planes, [&](int r, int a, int t) { return stat(r * kTileA + a, t).score; });
  }
  } while (select_next_tile(&tile, sel...));  // (the materialising and mask forms: one tile per workgroup)
  if constexpr (kSelect) select_finish(sel..., lists, planes);
}

// ================================================================ the transfer grid (transfer_grid.hip; grid_select.hip)
constexpr int kH1 = 256, kH2 = 128, kH3 = 64;

// ---- the prepared image, in floats.  W2 / W3 blocks are 64 lanes x 4 floats in A-operand order: lane l (row a = l & 31,
// half h = l >> 5), element b of block (g, mb) holds the kernel entry [input 8 g + 4 h + b][output 32 mb + a], so a
// lane's A operands of four consecutive k steps are one 16-byte load and a wave's load is 1 KB, contiguous.
constexpr int kImgW2 = 0;                          // [g 0..31][mb 0..3][64][4]
constexpr int kImgW3 = kImgW2 + kH1 * kH2;         // [kb 0..3][g 0..3][mb 0..1][64][4], input 32 kb + 8 g + 4 h + b
constexpr int kImgScale = kImgW3 + kH2 * kH3;      // gamma / sqrt(moving_var + eps)          [256]
constexpr int kImgShift = kImgScale + kH1;         // beta - moving_mean * scale              [256]
constexpr int kImgB2 = kImgShift + kH1;            // [128]
constexpr int kImgB3 = kImgB2 + kH2;               // [64]
constexpr int kImgWo = kImgB3 + kH3;               // [64]
constexpr int kImgBo = kImgWo + kH3;               // [1] + 3 pad
constexpr int kImgFloats = kImgBo + 4;             // 41 732 floats, 163.0 KiB

// One workgroup owns kTgTileC cations x kTgTileA anions; a wave owns two cations of the tile, i.e. two
// MFMA column blocks of 32 pairs (lane & 31 = anion), and fetches every weight once for its 64 pairs.
constexpr int kTgTileC = 8, kTgTileA = 32;
// Row stride (floats) of the anion u rows in LDS.  A lane reads its anion's row 16 bytes at a time (ds_read_b128: 16
// lanes per LDS cycle, 64 banks), so the 16 lanes of a group must start 4 banks apart: stride = 4 * odd.  256 unpadded
// would put every lane on one bank quad; 260 = 4 * 65.  The cation rows, scale and shift are read at one address per
// lane half (a broadcast), so they stay unpadded.
constexpr int kTgAnStride = kH1 + 4;
constexpr int kTgLdsFloats = kTgTileA * kTgAnStride + kTgTileC * kH1 + 2 * kH1 + kTgTileC * kTgTileA;  // 43.5 KiB

// The transfer grid's tile as partners: a 32-lane half of a wave is one tile row of `res`; then one thread per tile
// column walks its rows.
template <class Live>
__device__ __forceinline__ void partners_transfer_tile(const GridPartners& g, const float* res, int C, int A, int c0,
                                                       int a0, int nc, int na, int tiles_a, Live live) {
  const int tid = threadIdx.x, r = tid >> 5, p = tid & 31;
  const int ta = a0 / kTgTileA, tc = c0 / kTgTileC;
  const bool ok = r < nc && p < na && live(r, p);
  const unsigned long long entry = partners_entry(g, ok, res[tid], (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + p));
  partners_row<kTgTileA>(g, entry, r < nc ? g.rows + ((size_t)ta * C + c0 + r) * g.m : nullptr);
  if (tid < na) {
    PartnersBest best;
    for (int rr = 0; rr < nc; ++rr)
      best.offer(partners_entry(g, live(rr, tid), res[rr * kTgTileA + tid], (uint32_t)(c0 + rr) * (uint32_t)A + (uint32_t)(a0 + tid)));
    best.store(g.cols + ((size_t)tc * A + a0 + tid) * g.m, g.m);
  }
}

// The transfer grid's tile as summary records: a 32-lane half of a wave is one tile row of `res`; then one thread per
// tile column walks its rows in ascending order.
template <class Live>
__device__ __forceinline__ void summary_transfer_tile(const GridSummary& g, const float* res, int C, int A, int c0, int a0,
                                                      int nc, int na, int tiles_a, Live live) {
  const int tid = threadIdx.x, r = tid >> 5, p = tid & 31;
  const int ta = a0 / kTgTileA, tc = c0 / kTgTileC;
  const float v = res[tid];
  summary_row<kTgTileA>(r < nc && p < na && live(r, p) && v == v, v, r < nc ? g.rows + (size_t)ta * C + c0 + r : nullptr);
  if (tid < na) {
    SummarySum sum;
    for (int rr = 0; rr < nc; ++rr) {
      const float w = res[rr * kTgTileA + tid];
      sum.add(live(rr, tid) && w == w, w);
    }
    g.cols[(size_t)tc * A + a0 + tid] = sum.record();
  }
}

// The transfer grid's tile counted and as best-k mask words: thread tid holds pair (tid >> 5, tid & 31) of `res`; a wave's
// lanes are two tile rows of 32 anions, lane 0 and lane 32 each write the word of their own row.
template <class Live>
__device__ __forceinline__ void rank_transfer_tile(const GridRank& g, float* lists, const float* res, int, int A, int c0,
                                                   int a0, int nc, int na, Live live) {
  const int tid = threadIdx.x, r = tid >> 5, p = tid & 31;
  const bool ok = r < nc && p < na && live(r, p);
  rank_count(g, reinterpret_cast<uint32_t*>(lists), rank_prefix(g, 0), ok,
             rank_entry(res[tid], g.largest, (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + p)));
  __syncthreads();  // the tile's regions and mask words are free for the next tile
}
template <class Live>
__device__ __forceinline__ void rank_transfer_tile(const GridMaskRank& g, float*, const float* res, int, int A, int c0,
                                                   int a0, int nc, int na, Live live) {
  const int tid = threadIdx.x, r = tid >> 5, p = tid & 31;
  const bool ok = r < nc && p < na && live(r, p);
  const unsigned long long entry = rank_entry(res[tid], g.largest, (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + p));
  uint32_t* word = g.words + (int64_t)(c0 + r) * g.W + (a0 >> 5);
  mask_store_ballot(ok && entry <= g.state[0].bound, r < nc ? word : nullptr, r < nc ? word : nullptr);
}

__device__ __forceinline__ f32x16_t mfma32(float a, float b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Writes `rows` spans of `span` floats (row r starts at out + first + r * pitch, its values at res + r * rs) with
// 16-byte stores on every naturally aligned quad inside the span and 4-byte stores on the ragged ends (the scheme of
// head_grid.hip's store_rows, one value per pair).
__device__ __forceinline__ void store_spans(float* __restrict__ out, int64_t first, int64_t pitch, int rows, int span,
                                            const float* res, int rs) {
  const int64_t po = (int64_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
  const int quads = (span + 3) / 4 + 1;  // quads a span can touch at any alignment
  for (int item = threadIdx.x; item < rows * quads; item += blockDim.x) {
    const int r = item / quads, q = item - r * quads;
    const int64_t g0 = first + (int64_t)r * pitch;
    const int e0 = 4 * q - (int)((g0 + po) & 3);  // out + g0 + e0 is 16-byte aligned
    if (e0 >= span) continue;
    const float* v = res + r * rs + e0;
    if (e0 >= 0 && e0 + 3 < span) {
      // written once and not read again by the launch: a streaming (nontemporal) global_store_dwordx4
      __builtin_nontemporal_store(f32x4_t{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4_t*>(out + g0 + e0));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k >= 0 && e0 + k < span) out[g0 + e0 + k] = v[k];
    }
  }
}

// One k group (8 input features: 4 per lane half) of Dense 128 for a wave's two column blocks: the operand
// bn(relu(u_cat + u_an)) is formed in registers, then 4 k steps x 4 row blocks x 2 column blocks of MFMA.
__device__ __forceinline__ void dense128_group(f32x16_t (&acc)[4][2], const f32x4_t (&w)[4], const float* ua_row,
                                               const float* uc_row, const float* bn_half, int g) {
  const f32x4_t ua = ld4(ua_row + 8 * g), sc = ld4(bn_half + 8 * g), sh = ld4(bn_half + kH1 + 8 * g);
  const f32x4_t uc0 = ld4(uc_row + 8 * g), uc1 = ld4(uc_row + kH1 + 8 * g);
  float x[2][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {  // relu(mp_dense_1), then BatchNormalization's affine, per feature
    x[0][b] = fmaf(head_relu(uc0[b] + ua[b]), sc[b], sh[b]);
    x[1][b] = fmaf(head_relu(uc1[b] + ua[b]), sc[b], sh[b]);
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = mfma32(w[mb][b], x[nb][b], acc[mb][nb]);
}

// One k group of Dense 64: registers 4 g .. 4 g + 3 of the input block's accumulators, relu applied on the way.
__device__ __forceinline__ void dense64_group(f32x16_t (&acc)[2][2], const f32x16_t (&in)[2], const f32x4_t (&w)[2],
                                              int g) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float a2 = head_relu(in[nb][4 * g + b]);
      acc[0][nb] = mfma32(w[0][b], a2, acc[0][nb]);
      acc[1][nb] = mfma32(w[1][b], a2, acc[1][nb]);
    }
}

template <class... Sel>
__global__ __launch_bounds__(256) void transfer_grid_kernel(const float* __restrict__ u_cat,
                                                            const float* __restrict__ u_an,
                                                            const float* __restrict__ img, float* __restrict__ out,
                                                            int C, int A, int tiles_a, Sel... sel) {
  extern __shared__ __align__(16) float sm[];
  float* uan = sm;                            // [kTgTileA][kTgAnStride]
  float* ucat = uan + kTgTileA * kTgAnStride; // [kTgTileC][kH1]
  float* bnv = ucat + kTgTileC * kH1;         // scale kH1 | shift kH1
  float* res = bnv + 2 * kH1;                 // [kTgTileC][kTgTileA]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = lane & 31, h = lane >> 5;
  using Form = GridForm<Sel...>;
  constexpr bool kSelect = Form::select;
  unsigned tile = blockIdx.x;
  if constexpr (kSelect) select_init(sel..., sm + kTgLdsFloats, 1);
  if constexpr (Form::rank_count) rank_init(sel..., sm + kTgLdsFloats, 1);
  do {
  const int c0 = (tile / tiles_a) * kTgTileC, a0 = (tile % tiles_a) * kTgTileA;
  const int nc = min(kTgTileC, C - c0), na = min(kTgTileA, A - a0);
  if constexpr (Form::where) {  // a tile without a set bit: on to the next one, before any load
    if (!where_tile_any(sel..., sm + kTgLdsFloats, 1, c0, nc, a0 >> 5, kTgTileA / 32)) {
      if constexpr (Form::partners)  // (its slots have no other writer)
        partners_skip_tile(sel..., C, A, c0, a0, nc, na, tiles_a, a0 / kTgTileA, (C + kTgTileC - 1) / kTgTileC, c0 / kTgTileC, 1);
      continue;
    }
  }
  if constexpr (Form::rank_count || Form::rank_mask) {  // the rank forms' mask may be null: the same pass, when there is one
    if (rank_masked(sel...) && !where_tile_any(sel..., sm + kTgLdsFloats, 1, c0, nc, a0 >> 5, kTgTileA / 32)) {
      rank_skip_tile(sel..., C, c0, nc, a0 >> 5, kTgTileA / 32, 1);  // (its words have no other writer)
      continue;
    }
  }
  if constexpr (Form::summary) {  // the summary form's mask may be null too
    if (summary_masked(sel...) && !where_tile_any(sel..., sm + kTgLdsFloats, 1, c0, nc, a0 >> 5, kTgTileA / 32)) {
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
    const f32x4_t* w3 = reinterpret_cast<const f32x4_t*>(img + kImgW3) + lane;

    // Dense 128: the accumulators start at the bias (bias first, as every Dense of this project)
    f32x16_t acc2[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t bb = ld4(img + kImgB2 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc2[mb][0][4 * q + b] = acc2[mb][1][4 * q + b] = bb[b];
      }
    // The A operands of k group g + 1 travel while the 32 MFMAs of group g run: two register sets in turn, and
    // scheduling fences, without which the compiler sinks the loads to just before their use (one L2 latency exposed
    // per group).
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

    // Dense 64: the B operand of k step 4 g + b of input block kb is register 4 g + b of acc2[kb]
    f32x16_t acc3[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t bb = ld4(img + kImgB3 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc3[mb][0][4 * q + b] = acc3[mb][1][4 * q + b] = bb[b];
      }
    f32x4_t va[2], vb[2];
    va[0] = w3[0], va[1] = w3[64];
#pragma unroll
    for (int s = 0; s < 16; s += 2) {  // s = 4 kb + g
      vb[0] = w3[((s + 1) * 2 + 0) * 64], vb[1] = w3[((s + 1) * 2 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense64_group(acc3, acc2[s >> 2], va, s & 3);
      __builtin_amdgcn_sched_barrier(0);
      const int sn = s + 2 < 16 ? s + 2 : 15;
      va[0] = w3[(sn * 2 + 0) * 64], va[1] = w3[(sn * 2 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense64_group(acc3, acc2[(s + 1) >> 2], vb, (s + 1) & 3);
      __builtin_amdgcn_sched_barrier(0);
    }

    // Dense 1: a lane sums its 32 features in ascending order, the two lane halves meet (half 0 first), then the bias
    float part[2] = {0.f, 0.f};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t wo = ld4(img + kImgWo + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) part[nb] = fmaf(head_relu(acc3[mb][nb][4 * q + b]), wo[b], part[nb]);
      }
    const float bo = img[kImgBo];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float other = __shfl_xor(part[nb], 32);
      if (h == 0) res[(2 * wave + nb) * kTgTileA + p] = (part[nb] + other) + bo;
    }
  }
  __syncthreads();
  if constexpr (kSelect) {
    select_tile(sel..., sm + kTgLdsFloats, 1, kTgTileC * kTgTileA, [&](int, int, bool* live, uint32_t* pair) {
      const int r = tid >> 5;
      *live = r < nc && p < na;
      if constexpr (Form::where) *live = *live && where_bit(sel..., sm + kTgLdsFloats, 1, r, p, kTgTileA / 32);
      *pair = (uint32_t)(c0 + r) * (uint32_t)A + (uint32_t)(a0 + p);
      return res[tid];
    });
  } else if constexpr (Form::mask) {
    // a wave's lanes are two tile rows of 32 anions: lane 0 and lane 32 each write the word of their own row
    const int r = tid >> 5;
    const float v = res[tid];
    uint32_t* word = mask_word(sel..., c0 + r, a0 >> 5);
    mask_store_ballot(r < nc && p < na && mask_passes(sel..., v), r < nc ? word : nullptr, r < nc ? word : nullptr);
  } else if constexpr (Form::partners) {
    partners_transfer_tile(sel..., res, C, A, c0, a0, nc, na, tiles_a, [&](int r, int a) {
      if constexpr (Form::where) return where_bit(sel..., sm + kTgLdsFloats, 1, r, a, kTgTileA / 32);
      return true;
    });
  } else if constexpr (Form::rank_count || Form::rank_mask) {
    rank_transfer_tile(sel..., sm + kTgLdsFloats, res, C, A, c0, a0, nc, na, [&](int r, int a) {
      return !rank_masked(sel...) || where_bit(sel..., sm + kTgLdsFloats, 1, r, a, kTgTileA / 32);
    });
  } else if constexpr (Form::summary) {
    summary_transfer_tile(sel..., res, C, A, c0, a0, nc, na, tiles_a, [&](int r, int a) {
      return !summary_masked(sel...) || where_bit(sel..., sm + kTgLdsFloats, 1, r, a, kTgTileA / 32);
    });
  } else {
  store_spans(out, (int64_t)c0 * A + a0, (int64_t)A, nc, na, res, kTgTileA);
  }
  } while (select_next_tile(&tile, sel...));  // (the materialising form: one tile per workgroup)
  if constexpr (kSelect) select_finish(sel..., sm + kTgLdsFloats, 1);
  if constexpr (Form::rank_count) rank_finish(sel..., sm + kTgLdsFloats, 1);
}

// ================================================================ host side: the tile geometry and the one launcher
// Tiles along C, tiles along A and the tile's size for a family (0: head grid, 1: transfer grid, 2: ensemble grid - the
// head grid's tile, 3: transfer MC grid - the transfer grid's tile).
struct GridTiles {
  int tile_c, tile_a, c, a;
  int64_t count() const { return (int64_t)c * a; }
};
inline GridTiles grid_tiles(int family, int C, int A) {
  const bool head = family != 1 && family != 3;
  const int tc = head ? kTileC : kTgTileC, ta = head ? kTileA : kTgTileA;
  return {tc, ta, (C + tc - 1) / tc, (A + ta - 1) / ta};
}
// a workgroup per tile (the materialising and the mask-writing launches): the tiles must fit one launch
inline int grid_tiles_fit(const char* what, const GridTiles& t) {
  if (t.count() > 0x7fffffff)
    return fail(IMPNN_E_UNSUPPORTED, "%s: %lld tiles of %d x %d pairs exceed one launch; split the cation axis", what,
                (long long)t.count(), t.tile_c, t.tile_a);
  return IMPNN_OK;
}

// Where the materialising form of a family writes: out (every family; the ensemble's mean), params (the head grid's VFT
// parameters), std and score (the ensemble grid).  Null: not wanted; the other forms leave all of them null.
struct GridOut {
  float *out = nullptr, *params = nullptr, *std = nullptr, *score = nullptr;
};

// Every launch of head_grid_kernel / transfer_grid_kernel / ensemble_grid_kernel: `groups` workgroups, `extra_lds` bytes
// of dynamic LDS behind the tile's own, the trailing pack of the form (none: the materialising form, which alone takes
// `out`).  The kernel is picked here: kind 0 -> <0, 0>, kind 1 -> <1, 32> up to Mx = 32, else <1, 64>.  A request above
// 48 KiB raises the kernel's dynamic-LDS limit first.  FAMILY is a template argument so that a translation unit
// instantiates the kernels of the families it launches and no others.
template <int FAMILY, class... Sel>
void launch_grid_family(const GridOperands& g, unsigned groups, size_t extra_lds, const GridOut& out, Sel... sel) {
  const int tiles_a = grid_tiles(FAMILY, g.C, g.A).a;
  auto launch = [&](auto kern, size_t lds, auto... args) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kern<<<groups, 256, lds, g.stream>>>(args..., tiles_a, sel...);
  };
  if constexpr (FAMILY == 1) {
    launch(transfer_grid_kernel<Sel...>, sizeof(float) * kTgLdsFloats + extra_lds, g.mix_cat, g.mix_an, g.w, out.out, g.C, g.A);
  } else if constexpr (FAMILY == 2) {  // `w`: the members' tails
    const size_t lds = sizeof(float) * ensemble_lds_floats(g.kind, g.M, g.nT, g.F, g.Mx) + extra_lds;
    auto ens = [&](auto kern) {
      launch(kern, lds, g.mix_cat, g.mix_an, g.T, g.w, EnsembleOut{out.out, out.std, out.score}, g.M, g.kappa, g.C, g.A,
             g.nT, g.F, g.Mx);
    };
    if (g.kind == 0)
      ens(ensemble_grid_kernel<0, 0, Sel...>);
    else if (g.Mx <= 32)
      ens(ensemble_grid_kernel<1, 32, Sel...>);
    else
      ens(ensemble_grid_kernel<1, 64, Sel...>);
  } else {
    const float* tail = g.w + 2 * ((size_t)g.D * g.F + g.F) + 2 * ((size_t)g.F * g.Mx + g.Mx);  // behind the per-ion parts
    const size_t lds = sizeof(float) * grid_lds_floats(g.kind, g.nT, g.F, g.Mx) + extra_lds;
    auto head = [&](auto kern) { launch(kern, lds, g.mix_cat, g.mix_an, g.T, tail, out.out, out.params, g.C, g.A, g.nT, g.F, g.Mx); };
    if (g.kind == 0)
      head(head_grid_kernel<0, 0, Sel...>);
    else if (g.Mx <= 32)
      head(head_grid_kernel<1, 32, Sel...>);
    else
      head(head_grid_kernel<1, 64, Sel...>);
  }
}
// the selecting, mask-writing, partner and rank forms of the head and transfer grids: no output of the grid itself
template <class Sel>
void launch_grid_kernel(const GridOperands& g, unsigned groups, size_t extra_lds, const Sel& sel) {
  if (g.family == 0)
    launch_grid_family<0>(g, groups, extra_lds, GridOut{}, sel);
  else
    launch_grid_family<1>(g, groups, extra_lds, GridOut{}, sel);
}
// the transfer MC grid's kernel lives in transfer_mc_grid.hip: the tile launch of its summary form
void launch_transfer_mc_grid_summary_tiles(const GridOperands& g, unsigned groups, const GridSummary& sel);

}  // namespace impnn
