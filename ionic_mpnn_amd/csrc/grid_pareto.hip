// The Pareto filter of two objectives over a cation x anion grid (include/impnn.h: impnn_pareto_*): from two planes of
// float32 values to a short list of candidates that holds the whole front.
//
// A pair has the keys k1, k2 of its two values (select_key of grid_device.h: smaller is better).  The filter sorts the
// competing pairs into 2^kParetoBits buckets by k1 - bucket = (k1 - kmin) >> shift, the shift taken from the range the
// pairs really span - and keeps the smallest k2 of every bucket.  stair[b], the smallest k2 of the buckets below b,
// then belongs to a pair with a strictly smaller k1, so a pair of bucket b with stair[b] <= k2 is dominated by that
// pair and cannot be on the front: it is dropped.  What is left goes to the caller, who finishes the front.
//
// Stages, each one launch per row-block of the planes, in stream order, state in the caller's workspace:
//   begin      the key range, the bucket table and the counters are cleared
//   range      min and max of k1 and the number of competing pairs: a reduction per workgroup, then integer atomics
//   minima     persistent workgroups, each with a table of its own in LDS (LDS atomicMin), flushed once at the end:
//              the entries it touched, and of those only the ones below what the global table already shows
//   staircase  one workgroup: the exclusive prefix minimum of the table
//   collect    persistent workgroups with the staircase in LDS; survivors are appended through one counter add per
//              wave and element slot; the counter runs past the capacity, entries beyond it are not written
// Only integer atomics (min, max, add): range, table, counts and the candidate set do not depend on the schedule; the
// order of the candidate list does.  No workgroup waits for another.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kParetoBits = 14;
constexpr int kParetoBuckets = 1 << kParetoBits;  // 64 KiB of LDS: two workgroups fit a compute unit's 160 KiB
constexpr int kParetoBlock = 1024;                // threads of a streaming workgroup
constexpr int kParetoGroups = 256;                // persistent workgroups: one per compute unit of the MI355X
constexpr int kParetoRangeGroups = 1024;
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;        // no key: the image of no competing value

// the head of the workspace (impnn_pareto_header), then table [kParetoBuckets] and stair [kParetoBuckets]
struct ParetoState {
  uint32_t kmin, kmax;
  unsigned long long competing, candidates, reserved;
};
static_assert(sizeof(ParetoState) == sizeof(impnn_pareto_header), "the header is the state");

__host__ __device__ inline uint32_t* pareto_table(ParetoState* s) { return reinterpret_cast<uint32_t*>(s + 1); }
constexpr size_t kParetoWorkspaceBytes = sizeof(ParetoState) + 2 * sizeof(uint32_t) * kParetoBuckets;

// one row-block: n = rows * A values a plane, in units of four consecutive ones ("quads")
struct ParetoBlockArgs {
  const float* f1;
  const float* f2;
  const uint32_t* where;  // (rows, W) or null
  uint32_t n, A;
  int W, largest1, largest2, vec;  // vec: both planes 16-byte aligned, a whole quad is one load
};

__device__ __forceinline__ void load_quad(const float* p, uint32_t e0, uint32_t n, bool vec, float (&v)[4]) {
  if (vec && e0 + 4 <= n) {
    const f32x4_t q = ld4(p + e0);
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = e0 + i < n ? p[e0 + i] : __uint_as_float(0x7FC00000u);
  }
}

// fn(live, k1, k2, v1, v2, row, column) for the four elements of quad q, in order; every lane of the wave calls it
// (q may lie past the block: nothing is live then)
template <class Fn>
__device__ __forceinline__ void for_quad(const ParetoBlockArgs& b, uint32_t q, uint32_t quads, Fn&& fn) {
  const uint32_t e0 = q * 4u;
  float v1[4] = {0.f, 0.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t r = 0, j = 0;
  if (q < quads) {
    load_quad(b.f1, e0, b.n, b.vec != 0, v1);
    load_quad(b.f2, e0, b.n, b.vec != 0, v2);
    r = e0 / b.A, j = e0 - r * b.A;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bool live = q < quads && e0 + i < b.n && v1[i] == v1[i] && v2[i] == v2[i];
    if (live && b.where) live = (b.where[(size_t)r * b.W + (j >> 5)] >> (j & 31)) & 1u;
    fn(live, select_key(live ? v1[i] : 0.f, b.largest1 != 0), select_key(live ? v2[i] : 0.f, b.largest2 != 0),
       live ? v1[i] : 0.f, live ? v2[i] : 0.f, r, j);
    if (++j == b.A) j = 0, ++r;
  }
}

// the bucket of k1; a key outside the range of the range stage (planes that changed in between) lands in the last
// bucket: never outside the table
__device__ __forceinline__ uint32_t pareto_bucket(uint32_t k1, uint32_t kmin, int shift) {
  const uint32_t b = (k1 - kmin) >> shift;
  return b < (uint32_t)kParetoBuckets ? b : (uint32_t)kParetoBuckets - 1u;
}

__device__ __forceinline__ int pareto_shift(uint32_t kmin, uint32_t kmax) {
  const uint32_t span = kmax - kmin;
  const int length = span == 0 ? 0 : 32 - __clz((int)span);
  return length > kParetoBits ? length - kParetoBits : 0;
}

__global__ __launch_bounds__(256) void pareto_begin_kernel(ParetoState* s) {
  uint32_t* table = pareto_table(s);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * kParetoBuckets; i += gridDim.x * blockDim.x) table[i] = kKeyNone;
  if (blockIdx.x == 0 && threadIdx.x == 0) s->kmin = kKeyNone, s->kmax = 0u, s->competing = 0ull, s->candidates = 0ull, s->reserved = 0ull;
}

// a new collect round over the same staircase (larger candidate arrays): the candidate count alone
__global__ void pareto_restart_kernel(ParetoState* s) { s->candidates = 0ull; }

__global__ __launch_bounds__(kParetoBlock) void pareto_range_kernel(ParetoBlockArgs b, ParetoState* s) {
  __shared__ uint32_t part[3][kParetoBlock / kWave];
  const uint32_t quads = (b.n + 3u) >> 2;
  uint32_t lo = kKeyNone, hi = 0u, count = 0u;
  for (uint32_t q = blockIdx.x * kParetoBlock + threadIdx.x; q < quads; q += gridDim.x * kParetoBlock)
    for_quad(b, q, quads, [&](bool live, uint32_t k1, uint32_t, float, float, uint32_t, uint32_t) {
      if (live) lo = min(lo, k1), hi = max(hi, k1), ++count;
    });
  for (int step = kWave / 2; step > 0; step >>= 1) {
    lo = min(lo, (uint32_t)__shfl_xor((int)lo, step));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, step));
    count += (uint32_t)__shfl_xor((int)count, step);
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) part[0][wave] = lo, part[1][wave] = hi, part[2][wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kParetoBlock / kWave; ++w) lo = min(lo, part[0][w]), hi = max(hi, part[1][w]), count += part[2][w];
    if (count) {
      atomicMin(&s->kmin, lo);
      atomicMax(&s->kmax, hi);
      atomicAdd(&s->competing, (unsigned long long)count);
    }
  }
}

__global__ __launch_bounds__(kParetoBlock) void pareto_minima_kernel(ParetoBlockArgs b, ParetoState* s) {
  __shared__ uint32_t mine[kParetoBuckets];
  for (int i = threadIdx.x; i < kParetoBuckets; i += kParetoBlock) mine[i] = kKeyNone;
  const uint32_t kmin = s->kmin;
  const int shift = pareto_shift(kmin, s->kmax);
  const uint32_t quads = (b.n + 3u) >> 2;
  __syncthreads();
  for (uint32_t q = blockIdx.x * kParetoBlock + threadIdx.x; q < quads; q += gridDim.x * kParetoBlock)
    for_quad(b, q, quads, [&](bool live, uint32_t k1, uint32_t k2, float, float, uint32_t, uint32_t) {
      if (live) atomicMin(&mine[pareto_bucket(k1, kmin, shift)], k2);
    });
  __syncthreads();
  uint32_t* table = pareto_table(s);
  for (int i = threadIdx.x; i < kParetoBuckets; i += kParetoBlock) {
    const uint32_t k2 = mine[i];
    // the table only falls: a stale read is a larger one and costs an atomic, never a minimum
    if (k2 != kKeyNone && k2 < __hip_atomic_load(table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(table + i, k2);
  }
}

// stair[b] = min over buckets below b, kKeyNone for b = 0: thread t owns kParetoBuckets / blockDim.x consecutive buckets
__global__ __launch_bounds__(kParetoBlock) void pareto_staircase_kernel(ParetoState* s) {
  constexpr int kPer = kParetoBuckets / kParetoBlock;
  __shared__ uint32_t scan[kParetoBlock];
  const uint32_t* table = pareto_table(s);
  uint32_t* stair = pareto_table(s) + kParetoBuckets;
  const int t = threadIdx.x;
  uint32_t own[kPer], low = kKeyNone;
#pragma unroll
  for (int i = 0; i < kPer; ++i) own[i] = table[t * kPer + i], low = min(low, own[i]);
  scan[t] = low;
  __syncthreads();
  for (int step = 1; step < kParetoBlock; step <<= 1) {  // inclusive prefix minimum over the threads
    const uint32_t below = t >= step ? scan[t - step] : kKeyNone;
    __syncthreads();
    scan[t] = min(scan[t], below);
    __syncthreads();
  }
  uint32_t run = t > 0 ? scan[t - 1] : kKeyNone;
#pragma unroll
  for (int i = 0; i < kPer; ++i) stair[t * kPer + i] = run, run = min(run, own[i]);
}

__global__ __launch_bounds__(kParetoBlock) void pareto_collect_kernel(ParetoBlockArgs b, ParetoState* s, uint32_t row0,
                                                                      float* __restrict__ values, int32_t* __restrict__ cation,
                                                                      int32_t* __restrict__ anion, unsigned long long capacity) {
  __shared__ uint32_t stair[kParetoBuckets];
  const uint32_t* src = pareto_table(s) + kParetoBuckets;
  for (int i = threadIdx.x; i < kParetoBuckets; i += kParetoBlock) stair[i] = src[i];
  const uint32_t kmin = s->kmin;
  const int shift = pareto_shift(kmin, s->kmax);
  const uint32_t quads = (b.n + 3u) >> 2;
  const int lane = threadIdx.x % kWave;
  __syncthreads();
  // the bound is the wave's: every lane of a wave reaches the ballots
  for (uint32_t q0 = blockIdx.x * kParetoBlock + (threadIdx.x - lane); q0 < quads; q0 += gridDim.x * kParetoBlock)
    for_quad(b, q0 + lane, quads, [&](bool live, uint32_t k1, uint32_t k2, float v1, float v2, uint32_t r, uint32_t j) {
      const bool keep = live && !(stair[pareto_bucket(k1, kmin, shift)] <= k2);
      const unsigned long long votes = __ballot(keep);
      if (votes == 0ull) return;
      const int leader = __ffsll((long long)votes) - 1;
      unsigned long long base = 0ull;
      if (lane == leader) base = atomicAdd(&s->candidates, (unsigned long long)__popcll(votes));
      base = __shfl(base, leader);
      const unsigned long long slot = base + __popcll(votes & ((1ull << lane) - 1ull));
      if (keep && slot < capacity) {
        values[2 * slot] = v1, values[2 * slot + 1] = v2;
        cation[slot] = (int32_t)(row0 + r), anion[slot] = (int32_t)j;
      }
    });
}

// ---- the checks of the entries, in the order include/impnn.h gives
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int workspace_rule(const char* fn, const void* workspace, size_t bytes, bool null_checked) {
  if (!null_checked && !workspace) return fail(IMPNN_E_BADARG, "%s: null pointer", fn);
  if (!aligned(workspace, 8)) return fail(IMPNN_E_BADARG, "%s: the workspace must be 8-byte aligned", fn);
  if (bytes < kParetoWorkspaceBytes)
    return fail(IMPNN_E_WORKSPACE, "%s: workspace of %zu bytes is too small (%zu needed)", fn, bytes, kParetoWorkspaceBytes);
  return IMPNN_OK;
}

struct ParetoCall {
  const float* f1;
  const float* f2;
  const uint32_t* where;
  int largest1, largest2;
  void* workspace;
  size_t workspace_bytes;
  int rows, A;
  // collect alone
  bool collect;
  int64_t row0, capacity;
  const void* out[3];
};

// IMPNN_OK with *work = false: zero work
int pareto_checked(const char* fn, const ParetoCall& c, bool* work) {
  *work = false;
  if (c.rows < 0 || c.A < 0 || (c.collect && (c.row0 < 0 || c.capacity < 0))) return fail(IMPNN_E_BADARG, "%s: bad shape", fn);
  if ((c.largest1 | c.largest2) & ~1) return fail(IMPNN_E_BADARG, "%s: largest must be 0 or 1", fn);
  if (c.rows == 0 || c.A == 0) return IMPNN_OK;
  if (!c.f1 || !c.f2 || !c.workspace || (c.collect && c.capacity > 0 && !(c.out[0] && c.out[1] && c.out[2])))
    return fail(IMPNN_E_BADARG, "%s: null pointer", fn);
  if (!aligned(c.f1, 4) || !aligned(c.f2, 4) || !aligned(c.where, 4) || !aligned(c.out[0], 4) || !aligned(c.out[1], 4) ||
      !aligned(c.out[2], 4))
    return fail(IMPNN_E_BADARG, "%s: planes, mask and outputs must be 4-byte aligned", fn);
  if (int rc = workspace_rule(fn, c.workspace, c.workspace_bytes, true)) return rc;
  if ((int64_t)c.rows * c.A > INT32_MAX)
    return fail(IMPNN_E_UNSUPPORTED, "%s: %lld pairs in one row-block, at most 2^31 - 1", fn, (long long)c.rows * c.A);
  if (c.collect && c.row0 + c.rows > INT32_MAX)
    return fail(IMPNN_E_UNSUPPORTED, "%s: rows up to %lld, a cation index has 31 bits", fn, (long long)(c.row0 + c.rows));
  *work = true;
  return IMPNN_OK;
}

ParetoBlockArgs block_args(const ParetoCall& c) {
  return ParetoBlockArgs{c.f1, c.f2, c.where, (uint32_t)((int64_t)c.rows * c.A), (uint32_t)c.A, mask_row_words(c.A),
                         c.largest1, c.largest2, aligned16(c.f1) && aligned16(c.f2)};
}

unsigned pareto_groups(const ParetoBlockArgs& b, int most) {
  const uint32_t quads = (b.n + 3u) >> 2, want = (quads + kParetoBlock - 1) / kParetoBlock;
  return want < (uint32_t)most ? want : (uint32_t)most;
}

}  // namespace

}  // namespace impnn

using namespace impnn;

extern "C" {

int32_t impnn_pareto_bucket_bits(void) { return kParetoBits; }

int impnn_pareto_workspace_bytes(size_t* need) {
  if (!need) return fail(IMPNN_E_BADARG, "%s: null pointer", __func__);
  *need = kParetoWorkspaceBytes;
  return IMPNN_OK;
}

int impnn_pareto_begin(void* workspace, size_t workspace_bytes, impnn_stream_t stream) {
  if (int rc = workspace_rule(__func__, workspace, workspace_bytes, false)) return rc;
  pareto_begin_kernel<<<2 * kParetoBuckets / 256, 256, 0, as_stream(stream)>>>(static_cast<ParetoState*>(workspace));
  return check_launch("pareto_begin");
}

int impnn_pareto_range(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                       void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream) {
  const ParetoCall c{f1, f2, where, largest1, largest2, workspace, workspace_bytes, rows, A, false, 0, 0, {nullptr, nullptr, nullptr}};
  bool work;
  if (int rc = pareto_checked(__func__, c, &work)) return rc;
  if (!work) return IMPNN_OK;
  const ParetoBlockArgs b = block_args(c);
  pareto_range_kernel<<<pareto_groups(b, kParetoRangeGroups), kParetoBlock, 0, as_stream(stream)>>>(b, static_cast<ParetoState*>(workspace));
  return check_launch("pareto_range");
}

int impnn_pareto_minima(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                        void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream) {
  const ParetoCall c{f1, f2, where, largest1, largest2, workspace, workspace_bytes, rows, A, false, 0, 0, {nullptr, nullptr, nullptr}};
  bool work;
  if (int rc = pareto_checked(__func__, c, &work)) return rc;
  if (!work) return IMPNN_OK;
  const ParetoBlockArgs b = block_args(c);
  pareto_minima_kernel<<<pareto_groups(b, kParetoGroups), kParetoBlock, 0, as_stream(stream)>>>(b, static_cast<ParetoState*>(workspace));
  return check_launch("pareto_minima");
}

int impnn_pareto_staircase(void* workspace, size_t workspace_bytes, impnn_stream_t stream) {
  if (int rc = workspace_rule(__func__, workspace, workspace_bytes, false)) return rc;
  pareto_staircase_kernel<<<1, kParetoBlock, 0, as_stream(stream)>>>(static_cast<ParetoState*>(workspace));
  return check_launch("pareto_staircase");
}

int impnn_pareto_collect(const float* f1, const float* f2, const uint32_t* where, int32_t largest1, int32_t largest2,
                         int64_t row0, int32_t restart, float* values, int32_t* cation, int32_t* anion, int64_t capacity,
                         void* workspace, size_t workspace_bytes, int32_t rows, int32_t A, impnn_stream_t stream) {
  const ParetoCall c{f1, f2, where, largest1, largest2, workspace, workspace_bytes, rows, A, true, row0, capacity, {values, cation, anion}};
  bool work;
  if (int rc = pareto_checked(__func__, c, &work)) return rc;
  if (!work) return IMPNN_OK;
  ParetoState* s = static_cast<ParetoState*>(workspace);
  if (restart) {
    pareto_restart_kernel<<<1, 1, 0, as_stream(stream)>>>(s);
    if (int rc = check_launch("pareto_collect")) return rc;
  }
  const ParetoBlockArgs b = block_args(c);
  pareto_collect_kernel<<<pareto_groups(b, kParetoGroups), kParetoBlock, 0, as_stream(stream)>>>(
      b, s, (uint32_t)row0, values, cation, anion, (unsigned long long)capacity);
  return check_launch("pareto_collect");
}

}  // extern "C"
