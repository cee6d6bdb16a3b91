// The optimizer step: what Adam(1e-3, clipnorm=1.0) does for the reference's model.fit
// (train_viscosity.py:227-230, 328-338; train_melting_point.py:205-208), with the step counter and the learning-rate
// schedule evaluated on the device so that a captured step replays with a new rate.  Every norm is a thread-strided sum
// reduced in a fixed order, and every workgroup of a variable forms the same one: the update is bitwise reproducible.
#include "kernel_device.h"

namespace impnn {
namespace {

// ---------------------------------------------------------------------------------------
// Optimizer step: keras.optimizers.Adam(lr, clipnorm) as the trainers configure it
// (train_viscosity.py:227-230).  kAdamSplit workgroups per variable: each forms the variable's gradient norm itself
// (the same thread-strided sum in the same order in every workgroup, so all of them scale by the identical factor - no
// partials buffer, no second launch) and updates its own 1/kAdamSplit of the elements; with one workgroup per variable
// the step took as long as one workgroup needs for the largest variable (172 us at atom_dim 128: bond_transform, 131 K
// floats through one workgroup's 20 GB/s):
//   g <- g * clipnorm / max(||g||_2, clipnorm)          (tf.clip_by_norm, per variable; clipnorm <= 0: off)
//   m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2
//   w <- w - lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
// The variable table holds device pointers: 4 per variable (w, g, m, v) and the element count.
// ---------------------------------------------------------------------------------------
__global__ void incr_step_kernel(long long* step) { *step += 1; }
constexpr int kAdamSplit = 16;

// The learning rate of update number s (s updates already applied) from the 32-word record of impnn.h
// (impnn_adam_step_scheduled); every value in it is uniform, so the loads are scalar.  An unknown kind gives NaN.
__device__ __forceinline__ float lr_schedule_rate(const int* __restrict__ rec, long long s) {
  const int kind = rec[kLrKind];
  const float lr0 = __int_as_float(rec[kLrBase]);
  if (kind == kLrConstant) return lr0;
  if (kind == kLrExponential) {
    float p = (float)s / (float)rec[kLrDecaySteps];
    if (rec[kLrFlags] & 1) p = floorf(p);  // staircase
    return lr0 * powf(__int_as_float(rec[kLrParam]), p);
  }
  if (kind == kLrCosine) {
    const long long warm = rec[kLrWarmupSteps], dsteps = rec[kLrDecaySteps];
    const float target = __int_as_float(rec[kLrTarget]), alpha = __int_as_float(rec[kLrParam]);
    if (s < warm) return (target - lr0) * ((float)s / (float)warm) + lr0;
    const long long sp = s - warm < dsteps ? s - warm : dsteps;
    const float c = 0.5f * (1.0f + cosf(3.14159265358979323846f * ((float)sp / (float)dsteps)));
    return target * ((1.0f - alpha) * c + alpha);
  }
  if (kind == kLrPiecewise) {
    int nb = rec[kLrBoundaryCount];
    nb = nb < 0 ? 0 : nb > kLrMaxBoundaries ? kLrMaxBoundaries : nb;
    int i = 0;
    while (i < nb && s > (long long)rec[kLrBoundaries + i]) ++i;
    return __int_as_float(rec[kLrValues + i]);
  }
  return __int_as_float(0x7fc00000);
}

__global__ void lr_schedule_eval_kernel(const int* __restrict__ rec, const long long* __restrict__ steps,
                                        float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = lr_schedule_rate(rec, steps[i]);
}

// What impnn_adam_step_scheduled adds to the operands of the update kernel; the plain instantiation reads none of it.
struct AdamExtras {
  const int* rec;          // learning-rate record
  const float* partials;   // kGlobal: n_vars * kAdamSplit sums of squares (adam_sumsq_kernel)
  const int* decay_flags;  // kDecay: one word per variable, non-zero = the variable decays
  float global_clipnorm, weight_decay;
};

// The [lo, hi) of workgroup y of a variable of n elements: the update kernel and the sum-of-squares kernel cut alike.
__device__ __forceinline__ void adam_slice(long long n, long long& lo, long long& hi) {
  long long per = (n + gridDim.y - 1) / gridDim.y;
  if (per < 4096) per = 4096;  // small variables stay with their first workgroup(s)
  lo = (long long)blockIdx.y * per;
  hi = lo + per < n ? lo + per : n;
}

// global_clipnorm, first launch: partials[var * kAdamSplit + y] = sum of g^2 over slice y of variable var (0 for an
// empty slice), thread-strided and reduced in a fixed order.
__global__ __launch_bounds__(1024) void adam_sumsq_kernel(const unsigned long long* __restrict__ table,
                                                          const long long* __restrict__ sizes,
                                                          float* __restrict__ partials) {
  __shared__ float red[16];
  const int var = blockIdx.x;
  const float* g = reinterpret_cast<const float*>(table[4 * var + 1]);
  long long lo, hi;
  adam_slice(sizes[var], lo, hi);
  float ss = 0.f;
  for (long long t = lo + threadIdx.x; t < hi; t += blockDim.x) ss = fmaf(g[t], g[t], ss);
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += red[i];
    partials[(long long)var * gridDim.y + blockIdx.y] = tot;
  }
}

// kSched: the rate comes from the record and the device counter.  kGlobal: tf.clip_by_global_norm - every workgroup adds
// the partials itself, slices of a variable in slice order, then variables in variable order, so all of them hold the
// same bits; a non-finite norm gives the scale NaN (every update of the step is NaN, as in TensorFlow).  kDecay: keras's
// decoupled weight decay, w <- w - lr_t * wd * w ahead of the update, for the variables whose flag is set.
template <bool kSched, bool kGlobal, bool kDecay>
__global__ __launch_bounds__(1024) void adam_clipnorm_kernel(const unsigned long long* __restrict__ table,
                                                             const long long* __restrict__ sizes, float lr,
                                                             float b1, float b2, float eps, float clipnorm,
                                                             float corr1, float corr2,
                                                             const long long* __restrict__ step_dev, AdamExtras ex) {
  if (step_dev) {  // step counter in device memory (a captured hipGraph replays with a new step every time)
    const float t = (float)*step_dev;
    corr1 = 1.0f - powf(b1, t);
    corr2 = 1.0f - powf(b2, t);
  }
  if constexpr (kSched) lr = lr_schedule_rate(ex.rec, *step_dev - 1);  // keras: the schedule at `iterations` before the update
  __shared__ float red[16];
  __shared__ float scale_s;
  const int var = blockIdx.x;
  float* w = reinterpret_cast<float*>(table[4 * var + 0]);
  const float* g = reinterpret_cast<const float*>(table[4 * var + 1]);
  float* m = reinterpret_cast<float*>(table[4 * var + 2]);
  float* v = reinterpret_cast<float*>(table[4 * var + 3]);
  const long long n = sizes[var];
  if ((long long)blockIdx.y * 4096 >= n && blockIdx.y > 0) return;  // no elements for this workgroup
  if constexpr (kGlobal) {
    __shared__ float var_s[1024];
    const int nv = gridDim.x;
    float tot = 0.f;  // (thread 0's is the sum)
    for (int base = 0; base < nv; base += 1024) {
      const int q = base + (int)threadIdx.x;
      if (q < nv) {
        float a = 0.f;
        for (int k = 0; k < kAdamSplit; ++k) a += ex.partials[(long long)q * kAdamSplit + k];
        var_s[threadIdx.x] = a;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int cnt = nv - base < 1024 ? nv - base : 1024;
        for (int i = 0; i < cnt; ++i) tot += var_s[i];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float norm = sqrtf(tot), c = ex.global_clipnorm;
      scale_s = norm - norm == 0.f ? c / fmaxf(norm, c) : __int_as_float(0x7fc00000);  // (inf - inf, nan - nan: NaN)
    }
  } else {
    float ss = 0.f;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {  // 16-byte loads (every workgroup of the variable takes this path or none)
      const long long n4 = n >> 2;
      for (long long t = threadIdx.x; t < n4; t += blockDim.x) {
        const f32x4_t x = ldv4(g + 4 * t);
        ss = fmaf(x[0], x[0], ss);
        ss = fmaf(x[1], x[1], ss);
        ss = fmaf(x[2], x[2], ss);
        ss = fmaf(x[3], x[3], ss);
      }
      for (long long t = 4 * n4 + threadIdx.x; t < n; t += blockDim.x) ss = fmaf(g[t], g[t], ss);
    } else {
      for (long long t = threadIdx.x; t < n; t += blockDim.x) ss = fmaf(g[t], g[t], ss);
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
      for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += red[i];
      const float norm = sqrtf(tot);
      scale_s = clipnorm > 0.f ? clipnorm / fmaxf(norm, clipnorm) : 1.0f;
    }
  }
  __syncthreads();
  const float sc = scale_s;
  const float alpha = lr * sqrtf(corr2) / corr1;  // corr1 = 1 - b1^t, corr2 = 1 - b2^t
  long long per = (n + gridDim.y - 1) / gridDim.y;
  if (per < 4096) per = 4096;  // small variables stay with their first workgroup(s)
  const long long lo = (long long)blockIdx.y * per, hi = lo + per < n ? lo + per : n;
  float decay = 0.f;
  if constexpr (kDecay) decay = ex.decay_flags[var] ? lr * ex.weight_decay : 0.f;
  for (long long t = lo + threadIdx.x; t < hi; t += blockDim.x) {
    const float gg = g[t] * sc;
    const float mm = b1 * m[t] + (1.0f - b1) * gg;
    const float vv = b2 * v[t] + (1.0f - b2) * gg * gg;
    m[t] = mm;
    v[t] = vv;
    if constexpr (kDecay) {
      const float ww = w[t];
      w[t] = (decay != 0.f ? ww - ww * decay : ww) - alpha * mm / (sqrtf(vv) + eps);
    } else {
      w[t] -= alpha * mm / (sqrtf(vv) + eps);
    }
  }
}

}  // namespace

int launch_adam_clipnorm(const void* table, const void* sizes, int n_vars, int64_t step, int64_t* step_dev, float lr,
                         float b1, float b2, float eps, float clipnorm, hipStream_t s) {
  float corr1 = 1.0f, corr2 = 1.0f;
  if (step_dev) {
    incr_step_kernel<<<1, 1, 0, s>>>(reinterpret_cast<long long*>(step_dev));
    if (int rc = check_launch("incr_step")) return rc;
  } else {
    corr1 = 1.0f - powf(b1, (float)step);
    corr2 = 1.0f - powf(b2, (float)step);
  }
  adam_clipnorm_kernel<false, false, false><<<dim3(n_vars, kAdamSplit), 1024, 0, s>>>(
      static_cast<const unsigned long long*>(table), static_cast<const long long*>(sizes), lr, b1, b2, eps, clipnorm,
      corr1, corr2, reinterpret_cast<const long long*>(step_dev), AdamExtras{});
  return check_launch("adam_clipnorm");
}

int64_t adam_scheduled_workspace(int n_vars) { return (int64_t)(n_vars > 0 ? n_vars : 0) * kAdamSplit; }

int launch_adam_scheduled(const void* table, const void* sizes, int n_vars, int64_t* step_dev, const void* record,
                          float b1, float b2, float eps, float clipnorm, float global_clipnorm, float weight_decay,
                          const int32_t* decay_flags, float* partials, hipStream_t s) {
  const auto* tb = static_cast<const unsigned long long*>(table);
  const auto* sz = static_cast<const long long*>(sizes);
  const auto* sd = reinterpret_cast<const long long*>(step_dev);
  const bool global = global_clipnorm > 0.f, decay = decay_flags != nullptr;
  incr_step_kernel<<<1, 1, 0, s>>>(reinterpret_cast<long long*>(step_dev));
  if (int rc = check_launch("incr_step")) return rc;
  if (global) {  // the one extra launch: per-(variable, slice) sums of squares
    adam_sumsq_kernel<<<dim3(n_vars, kAdamSplit), 1024, 0, s>>>(tb, sz, partials);
    if (int rc = check_launch("adam_sumsq")) return rc;
  }
  const AdamExtras ex{static_cast<const int*>(record), partials, decay_flags, global_clipnorm, weight_decay};
  const dim3 grid(n_vars, kAdamSplit);
#define ADAM_SCHEDULED(G, W) \
  adam_clipnorm_kernel<true, G, W><<<grid, 1024, 0, s>>>(tb, sz, 0.f, b1, b2, eps, clipnorm, 1.0f, 1.0f, sd, ex)
  if (global && decay) ADAM_SCHEDULED(true, true);
  else if (global) ADAM_SCHEDULED(true, false);
  else if (decay) ADAM_SCHEDULED(false, true);
  else ADAM_SCHEDULED(false, false);
#undef ADAM_SCHEDULED
  return check_launch("adam_scheduled");
}

int launch_lr_schedule_eval(const void* record, const int64_t* steps, float* out, int n, hipStream_t s) {
  lr_schedule_eval_kernel<<<(n + 255) / 256, 256, 0, s>>>(static_cast<const int*>(record),
                                                         reinterpret_cast<const long long*>(steps), out, n);
  return check_launch("lr_schedule_eval");
}

}  // namespace impnn
