// Segmented regression sums (include/impnn.h, impnn_regression_sums): (pred, y, w) -> per segment an 8-word fp64
// record from which MAE, MSE, RMSE, bias, the maximal error and R^2 follow on the host.  DESIGN.md 6.1.3.
//
// A group of kGroup threads owns one segment.  Summation order, the same at every call of one (n, n_seg):
//   1. thread t adds its elements k = lo + t, lo + t + kGroup, ... in that order (fp64);
//   2. the 64 lanes of a wave fold by halves: lane l takes lane l + 32, then l + 16, ... l + 1 (an fp64 value crosses
//      lanes as two 32-bit moves);
//   3. the group's waves are added in wave order by the thread that owns the word;
//   4. thread j < 8 of the group owns word j and does the read-modify-write on `sums` (stream order: no atomic).
// No workgroup shares a segment with another one, so there is no cross-workgroup step and no workspace.
#include "common.h"

#pragma clang fp contract(off)  // every term is the product numpy forms: no product is fused into the sum behind it

namespace impnn {
namespace {

constexpr int kSumWords = 8;

struct RegressionSumsCall {
  const float *pred, *y, *w;
  const int32_t* order;
  const int64_t* seg_offsets;
  int64_t n;
  int32_t n_seg;
  double offset, scale;
  int accumulate;
  double* sums;
};

__device__ __forceinline__ double lane_down(double v, int d) {
  const int lo = __shfl_down(__double2loint(v), d), hi = __shfl_down(__double2hiint(v), d);
  return __hiloint2double(hi, lo);
}

// the maximum that keeps a NaN (fmax drops it)
__device__ __forceinline__ double max_keep_nan(double a, double b) { return (a != a || b > a) ? a != a ? a : b : (b != b ? b : a); }

template <int kGroup, int kBlock>
__global__ __launch_bounds__(kBlock) void regression_sums_kernel(RegressionSumsCall c) {
  constexpr int kGroups = kBlock / kGroup, kWaves = kGroup / kWave;
  __shared__ double part[kBlock / kWave][kSumWords];
  const int tid = threadIdx.x, g = tid / kGroup, t = tid % kGroup;
  const int64_t s = (int64_t)blockIdx.x * kGroups + g;
  const bool live = s < c.n_seg;
  int64_t lo = 0, hi = 0;
  if (live) {
    lo = c.seg_offsets ? c.seg_offsets[s] : 0;
    hi = c.seg_offsets ? c.seg_offsets[s + 1] : c.n;
    hi = hi < 0 ? 0 : hi > c.n ? c.n : hi;  // a segment never reaches outside the n samples, whatever the offsets hold
    lo = lo < 0 ? 0 : lo > hi ? hi : lo;
  }
  double a[kSumWords];
#pragma unroll
  for (int j = 0; j < kSumWords; ++j) a[j] = 0.0;
  for (int64_t k = lo + t; k < hi; k += kGroup) {
    const int64_t b = c.order ? (int64_t)c.order[k] : k;
    if ((uint64_t)b >= (uint64_t)c.n) continue;  // an index outside the arrays is not read
    const double p = (double)c.pred[b], yv = (double)c.y[b];
    const double w = c.w ? (double)c.w[b] : 1.0;
    const double e = c.scale * (p - yv);
    const double yr = c.offset + c.scale * yv;
    const double ae = fabs(e);
    a[1] += w;
    a[2] += w * e;
    a[3] += w * ae;
    a[4] += w * (e * e);
    a[5] += w * yr;
    a[6] += w * (yr * yr);
    if (w > 0.0) a[7] = max_keep_nan(a[7], ae);
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
#pragma unroll
    for (int j = 1; j < 7; ++j) a[j] += lane_down(a[j], d);
    a[7] = max_keep_nan(a[7], lane_down(a[7], d));
  }
  if ((tid & (kWave - 1)) == 0) {
    part[tid / kWave][0] = 0.0;
#pragma unroll
    for (int j = 1; j < kSumWords; ++j) part[tid / kWave][j] = a[j];
  }
  __syncthreads();
  if (live && t < kSumWords) {
    double v = part[g * kWaves][t];
    for (int wv = 1; wv < kWaves; ++wv) {
      const double o = part[g * kWaves + wv][t];
      v = t == 7 ? max_keep_nan(v, o) : v + o;
    }
    if (t == 0) v = (double)(hi - lo);
    double* dst = c.sums + s * kSumWords + t;
    if (c.accumulate) {
      const double old = *dst;
      v = t == 7 ? max_keep_nan(old, v) : old + v;
    }
    *dst = v;
  }
}

template <int kGroup, int kBlock>
int launch(const RegressionSumsCall& c, hipStream_t stream) {
  const int per_block = kBlock / kGroup;
  const unsigned blocks = (unsigned)(((int64_t)c.n_seg + per_block - 1) / per_block);
  hipLaunchKernelGGL((regression_sums_kernel<kGroup, kBlock>), dim3(blocks), dim3(kBlock), 0, stream, c);
  return check_launch("impnn_regression_sums");
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool is_finite(double x) { return x - x == 0.0; }

}  // namespace
}  // namespace impnn

using namespace impnn;

#define REQUIRE(cond, what)                                              \
  do {                                                                   \
    if (!(cond)) return fail(IMPNN_E_BADARG, "%s: %s", __func__, what); \
  } while (0)

extern "C" {

int64_t impnn_regression_sums_words(void) { return kSumWords; }

int impnn_regression_sums(const float* pred, const float* y, const float* sample_weight, const int32_t* order,
                          const int64_t* seg_offsets, int64_t n, int32_t n_seg, double offset, double scale,
                          int32_t accumulate, double* sums, impnn_stream_t stream) {
  REQUIRE(n >= 0, "n must be >= 0");
  REQUIRE(n_seg >= 1, "n_seg must be >= 1");
  REQUIRE(pred && y && sums, "null pointer (pred, y, sums)");
  REQUIRE(seg_offsets || n_seg == 1, "null seg_offsets with more than one segment");
  REQUIRE(aligned_to(pred, 4) && aligned_to(y, 4) && aligned_to(sample_weight, 4) && aligned_to(order, 4),
          "pred, y, sample_weight and order must be 4-byte aligned");
  REQUIRE(aligned_to(seg_offsets, 8) && aligned_to(sums, 8), "seg_offsets and sums must be 8-byte aligned");
  REQUIRE(is_finite(scale) && scale != 0.0, "scale must be finite and not zero");
  REQUIRE(is_finite(offset), "offset must be finite");
  REQUIRE(!order || n <= INT32_MAX, "order holds 32-bit indices: n must be below 2^31");
  hipStream_t st = as_stream(stream);
  if (n == 0 && n_seg == 1) {  // nothing to add; an overwriting call leaves the record of an empty segment
    if (!accumulate && hipMemsetAsync(sums, 0, kSumWords * sizeof(double), st) != hipSuccess)
      return fail(IMPNN_E_LAUNCH, "%s: hipMemsetAsync failed", __func__);
    return IMPNN_OK;
  }
  const RegressionSumsCall c{pred, y, sample_weight, order, seg_offsets, n, n_seg, offset, scale, accumulate != 0, sums};
  // the path follows (n, n_seg) alone, never the data: one call, one order of additions, one set of bits
  if (n_seg == 1) {
    if (n <= 64) return launch<64, 64>(c, st);       // a mini-batch of the captured step: one wave
    if (n <= 16384) return launch<256, 256>(c, st);  // one small workgroup
    return launch<1024, 1024>(c, st);                // one large workgroup: correct at any n, not fast
  }
  if (n / n_seg > 512) return launch<256, 256>(c, st);  // long segments on average: a workgroup each
  return launch<64, 256>(c, st);                        // the per-group table: a wave per segment
}

}  // extern "C"
