// The transfer-learning head (train_melting_point_transfer.py:95-103) behind GlobalSumPool, forward, loss and backward:
//   pooled_cat, pooled_an -> fp Dense relu (per ion) -> proj Dense relu (per ion) -> add
//     -> Dense 256 relu -> BatchNormalization -> Dense 128 relu -> Dropout -> Dense 64 relu -> Dense 1
//     -> Huber(delta) or squared error against y, mean over the batch (with sample weights: (1/B) sum_b w_b L_b),
//        + l2 penalties
// Tensor order of `weights` / `dweights` (kThTensors pointers, keras shapes: kernels (in,out)):
//   0 Wfp_cat 1 bfp_cat 2 Wfp_an 3 bfp_an 4 Wp_cat 5 bp_cat 6 Wp_an 7 bp_an 8 W1 9 b1 10 gamma 11 beta 12 W2 13 b2
//   14 W3 15 b3 16 Wo 17 bo
// The head's ~48 K weights (190 KB) do not fit LDS: a workgroup takes kThSPB samples at a time, holds their activations
// in LDS and streams each weight once per tile (every lane owns an output column, so the reads are coalesced and each
// value is used kThSPB times).  The batch statistics of BatchNormalization cut the forward and the backward in two:
//   forward, batch statistics:  th_forward(pre) -> th_bn_stats -> th_forward(post [+ loss])            3 launches
//   forward, moving statistics: th_forward(pre + post [+ loss])                                        1 launch
//   backward: th_bwd_post -> th_bn_bwd_stats (batch statistics only) -> th_bwd_pre -> th_param_grads   4 (3) launches
// Every sum that decides a forward value runs in a fixed order (no atomics): the same inputs give the same bits.
#include "common.h"

namespace impnn {
namespace {

constexpr int kThSPB = 8, kThThreads = 256;
constexpr int kThH1 = 256, kThH2 = 128, kThH3 = 64;
constexpr int kThStatLanes = 16;  // sample lanes per feature in the statistics kernels

struct ThTensors {
  const float* w[kThTensors];
};

// where the vectors of a pass live in `saved` (forward -> backward) and in the backward's workspace, in floats
struct ThSaved {
  int64_t fp, pr, mix, a1, bn, a2, a3, pred, stat, total;
};
__host__ __device__ inline ThSaved th_saved(int64_t B, int F, int Mx) {
  ThSaved o;
  o.fp = 0;
  o.pr = o.fp + B * 2 * F;
  o.mix = o.pr + B * 2 * Mx;
  o.a1 = o.mix + B * Mx;
  o.bn = o.a1 + B * kThH1;
  o.a2 = o.bn + B * kThH1;
  o.a3 = o.a2 + B * kThH2;
  o.pred = o.a3 + B * kThH3;
  o.stat = o.pred + B;  // mean[kThH1], inv_std[kThH1]
  o.total = o.stat + 2 * kThH1;
  return o;
}
struct ThWork {
  int64_t dz3, dz2, g, dz1, dpr, dfp, dpred, bst, total;
};
__host__ __device__ inline ThWork th_work(int64_t B, int F, int Mx) {
  ThWork o;
  o.dz3 = 0;
  o.dz2 = o.dz3 + B * kThH3;
  o.g = o.dz2 + B * kThH2;
  o.dz1 = o.g + B * kThH1;
  o.dpr = o.dz1 + B * kThH1;
  o.dfp = o.dpr + B * 2 * Mx;
  o.dpred = o.dfp + B * 2 * F;
  o.bst = o.dpred + B;  // mean_b g[kThH1], mean_b g * xhat [kThH1]
  o.total = o.bst + 2 * kThH1;
  return o;
}
__host__ __device__ inline int th_tensor_floats(int t, int D, int F, int Mx) {
  switch (t) {
    case 0: case 2: return D * F;
    case 1: case 3: return F;
    case 4: case 6: return F * Mx;
    case 5: case 7: return Mx;
    case 8: return Mx * kThH1;
    case 9: case 10: case 11: return kThH1;
    case 12: return kThH1 * kThH2;
    case 13: return kThH2;
    case 14: return kThH2 * kThH3;
    case 15: return kThH3;
    case 16: return kThH3;
    default: return 1;
  }
}

struct ThLoss {
  const float* y;         // (B); null: no loss
  float* loss_out;        // device scalar
  float* partial;         // one error sum per workgroup
  unsigned int* counter;  // arrival ticket: zero before the first call, left at zero by every call
  float l2[kThTensors];
  float delta;            // Huber's delta
  int kind;               // 0: squared error, 1: Huber
  float inv_B;
};
// With sample weights the loss is (1/B) sum_b w_b L_b, B counting the samples of weight 0 too.  The weights are the last
// argument of th_forward and th_bwd_post, which only their weighted instances look at: a call without them launches the
// instances that hold no weight instruction and no multiply by 1.

__device__ __forceinline__ float th_loss_value(int kind, float delta, float e) {
  if (kind == 0) return e * e;
  const float a = fabsf(e);
  return a <= delta ? 0.5f * e * e : delta * (a - 0.5f * delta);
}
__device__ __forceinline__ float th_loss_grad(int kind, float delta, float e) {
  if (kind == 0) return 2.0f * e;
  return fabsf(e) <= delta ? e : (e > 0.f ? delta : -delta);
}

struct ThSmem {
  float x[kThSPB * 2 * kHeadMaxX];
  float fp[kThSPB * 2 * kHeadMaxDim];
  float pr[kThSPB * 2 * kHeadMaxDim];
  float mix[kThSPB * kHeadMaxDim];
  float a1[kThSPB * kThH1];
  float bn[kThSPB * kThH1];
  float a2[kThSPB * kThH2];
  float a3[kThSPB * kThH3];
  float part[kThSPB * kThThreads];
  float small[kThSPB];
};

// out[s * os + o] = act(bias[o] + sum_k x[s * xs + k] * W[k * sk + o * so]) for the tile's kThSPB samples and o < J.
// J <= 256; x, out and part are LDS.  The k range is cut into 256 / J parts that run side by side; their partial sums
// are added in part order.  Ends with a barrier; the caller made x visible with one.
__device__ __forceinline__ void th_dense(const float* x, int xs, int K, const float* __restrict__ W, int sk, int so,
                                         const float* __restrict__ bias, int J, float* out, int os, bool relu,
                                         float* part) {
  const int tid = threadIdx.x;
  const int nparts = kThThreads / J;
  const int kchunk = (K + nparts - 1) / nparts;
  const int p = tid / J, o = tid - p * J;
  if (p < nparts) {
    float acc[kThSPB];
#pragma unroll
    for (int s = 0; s < kThSPB; ++s) acc[s] = 0.f;
    const int k0 = p * kchunk, k1 = min(K, k0 + kchunk);
#pragma unroll 4
    for (int k = k0; k < k1; ++k) {
      const float w = W[(int64_t)k * sk + (int64_t)o * so];
#pragma unroll
      for (int s = 0; s < kThSPB; ++s) acc[s] = fmaf(x[s * xs + k], w, acc[s]);
    }
#pragma unroll
    for (int s = 0; s < kThSPB; ++s) part[(p * kThSPB + s) * J + o] = acc[s];
  }
  __syncthreads();
  for (int idx = tid; idx < kThSPB * J; idx += kThThreads) {
    const int s = idx / J, oo = idx - s * J;
    float v = bias ? bias[oo] : 0.f;
    for (int q = 0; q < nparts; ++q) v += part[(q * kThSPB + s) * J + oo];
    out[s * os + oo] = relu ? fmaxf(v, 0.f) : v;
  }
  __syncthreads();
}

// deterministic workgroup sum of one value per thread; result valid in every thread
__device__ __forceinline__ float th_block_sum(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kThThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// copies a tile's [kThSPB][n] vectors between LDS (row stride ls) and global (rows b0.., row stride n)
__device__ __forceinline__ void th_store_tile(const float* lds, int ls, float* g, int n, int b0, int B) {
  for (int idx = threadIdx.x; idx < kThSPB * n; idx += kThThreads) {
    const int s = idx / n, j = idx - s * n;
    if (b0 + s < B) g[(int64_t)(b0 + s) * n + j] = lds[s * ls + j];
  }
}
__device__ __forceinline__ void th_load_tile(float* lds, int ls, const float* g, int n, int b0, int B) {
  for (int idx = threadIdx.x; idx < kThSPB * n; idx += kThThreads) {
    const int s = idx / n, j = idx - s * n;
    lds[s * ls + j] = b0 + s < B ? g[(int64_t)(b0 + s) * n + j] : 0.f;
  }
}

// flags of th_forward
enum { kThPre = 1, kThPost = 2, kThBatchStats = 4 };

// kWeighted: a loss call with sample weights (hl.y and hl.w set); the other instance has no trace of them.  The
// weights touch the loss only: BatchNormalization's statistics and the dropout masks do not see them.
// kRows: pc (C,D) and pa (A,D) are tables of ion rows and sample b reads pc[crow[b]], pa[arow[b]] (a stage-1 fit over
// cached encodings); an index outside its table reads a row of zeros.  Only the tile load differs: the other instances
// never look at crow / arow / C / A.
template <bool kWeighted, bool kRows>
__global__ __launch_bounds__(kThThreads) void th_forward(const float* __restrict__ pc, const float* __restrict__ pa,
                                                         ThTensors ht, const float* __restrict__ moving_mean,
                                                         const float* __restrict__ moving_var, float bn_eps, int flags,
                                                         float* __restrict__ saved, float* __restrict__ out, int B,
                                                         int D, int F, int Mx, bool dropout, DropoutArgs drop,
                                                         ThLoss hl, const float* __restrict__ sw,
                                                         const int* __restrict__ crow, const int* __restrict__ arow,
                                                         int C, int A) {
  __shared__ ThSmem sm;
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * kThSPB;
  const ThSaved so = th_saved(B, F, Mx);
  if (flags & kThPre) {
    for (int idx = tid; idx < kThSPB * 2 * D; idx += kThThreads) {
      const int s = idx / (2 * D), r = idx - s * 2 * D, g = r / D, i = r - g * D;
      if constexpr (kRows) {
        float v = 0.f;
        if (b0 + s < B) {
          const int row = (g == 0 ? crow : arow)[b0 + s];
          if ((unsigned)row < (unsigned)(g == 0 ? C : A)) v = (g == 0 ? pc : pa)[(int64_t)row * D + i];
        }
        sm.x[(s * 2 + g) * kHeadMaxX + i] = v;
      } else {
        sm.x[(s * 2 + g) * kHeadMaxX + i] = b0 + s < B ? (g == 0 ? pc : pa)[(int64_t)(b0 + s) * D + i] : 0.f;
      }
    }
    __syncthreads();
    for (int g = 0; g < 2; ++g)
      th_dense(sm.x + g * kHeadMaxX, 2 * kHeadMaxX, D, ht.w[2 * g], F, 1, ht.w[2 * g + 1], F, sm.fp + g * kHeadMaxDim,
               2 * kHeadMaxDim, true, sm.part);
    for (int g = 0; g < 2; ++g)
      th_dense(sm.fp + g * kHeadMaxDim, 2 * kHeadMaxDim, F, ht.w[4 + 2 * g], Mx, 1, ht.w[5 + 2 * g], Mx, sm.pr + g * kHeadMaxDim,
               2 * kHeadMaxDim, true, sm.part);
    for (int idx = tid; idx < kThSPB * Mx; idx += kThThreads) {
      const int s = idx / Mx, j = idx - s * Mx;
      sm.mix[s * kHeadMaxDim + j] = sm.pr[(s * 2) * kHeadMaxDim + j] + sm.pr[(s * 2 + 1) * kHeadMaxDim + j];
    }
    __syncthreads();
    th_dense(sm.mix, kHeadMaxDim, Mx, ht.w[8], kThH1, 1, ht.w[9], kThH1, sm.a1, kThH1, true, sm.part);
    if (saved) {
      for (int idx = tid; idx < kThSPB * 2 * F; idx += kThThreads) {
        const int s = idx / (2 * F), r = idx - s * 2 * F, g = r / F, j = r - g * F;
        if (b0 + s < B) saved[so.fp + (int64_t)(b0 + s) * 2 * F + r] = sm.fp[(s * 2 + g) * kHeadMaxDim + j];
      }
      for (int idx = tid; idx < kThSPB * 2 * Mx; idx += kThThreads) {
        const int s = idx / (2 * Mx), r = idx - s * 2 * Mx, g = r / Mx, j = r - g * Mx;
        if (b0 + s < B) saved[so.pr + (int64_t)(b0 + s) * 2 * Mx + r] = sm.pr[(s * 2 + g) * kHeadMaxDim + j];
      }
      th_store_tile(sm.mix, kHeadMaxDim, saved + so.mix, Mx, b0, B);
      th_store_tile(sm.a1, kThH1, saved + so.a1, kThH1, b0, B);
    }
  }
  if (!(flags & kThPost)) return;
  if (!(flags & kThPre)) th_load_tile(sm.a1, kThH1, saved + so.a1, kThH1, b0, B);
  {  // BatchNormalization: one feature per thread (kThH1 == kThThreads)
    float mean, inv_std;
    if (flags & kThBatchStats) {
      mean = saved[so.stat + tid], inv_std = saved[so.stat + kThH1 + tid];
    } else {
      mean = moving_mean[tid], inv_std = 1.0f / sqrtf(moving_var[tid] + bn_eps);
      if (saved && blockIdx.x == 0) saved[so.stat + tid] = mean, saved[so.stat + kThH1 + tid] = inv_std;
    }
    const float gam = ht.w[10][tid], bet = ht.w[11][tid];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kThSPB; ++s) sm.bn[s * kThH1 + tid] = (sm.a1[s * kThH1 + tid] - mean) * inv_std * gam + bet;
    __syncthreads();
  }
  th_dense(sm.bn, kThH1, kThH1, ht.w[12], kThH2, 1, ht.w[13], kThH2, sm.a2, kThH2, true, sm.part);
  if (dropout) {
    const DropoutKey key = dropout_key(drop);
    for (int idx = tid; idx < kThSPB * (kThH2 / 4); idx += kThThreads) {
      const int s = idx / (kThH2 / 4), c4 = idx - s * (kThH2 / 4);
      const Philox4 p = dropout_bits(key, b0 + s, c4);
#pragma unroll
      for (int q = 0; q < 4; ++q) sm.a2[s * kThH2 + 4 * c4 + q] = dropout_apply(key, p.v[q], sm.a2[s * kThH2 + 4 * c4 + q]);
    }
    __syncthreads();
  }
  th_dense(sm.a2, kThH2, kThH2, ht.w[14], kThH3, 1, ht.w[15], kThH3, sm.a3, kThH3, true, sm.part);
  th_dense(sm.a3, kThH3, kThH3, ht.w[16], 1, 1, ht.w[17], 1, sm.small, 1, false, sm.part);
  if (tid < kThSPB && b0 + tid < B) {
    if (out) out[b0 + tid] = sm.small[tid];
    if (saved) saved[so.pred + b0 + tid] = sm.small[tid];
  }
  if (saved) {
    th_store_tile(sm.bn, kThH1, saved + so.bn, kThH1, b0, B);
    th_store_tile(sm.a2, kThH2, saved + so.a2, kThH2, b0, B);
    th_store_tile(sm.a3, kThH3, saved + so.a3, kThH3, b0, B);
  }
  if (!hl.y) return;
  // ---- loss: workgroup sums in sample order, then the LAST workgroup to arrive adds them in workgroup order
  if (tid == 0) {
    float sum = 0.f;
    for (int s = 0; s < kThSPB; ++s)
      if (b0 + s < B) {
        if constexpr (kWeighted)
          sum += sw[b0 + s] * th_loss_value(hl.kind, hl.delta, sm.small[s] - hl.y[b0 + s]);
        else
          sum += th_loss_value(hl.kind, hl.delta, sm.small[s] - hl.y[b0 + s]);
      }
    __hip_atomic_store(&hl.partial[blockIdx.x], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const unsigned int ticket = atomicAdd(hl.counter, 1u);
    is_last = ticket == gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  float v = 0.f;
  for (int i = tid; i < (int)gridDim.x; i += kThThreads)
    v += __hip_atomic_load(&hl.partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float se = th_block_sum(v, sm.part);
  float reg = 0.f;
  for (int t = 0; t < kThTensors; ++t) {
    if (hl.l2[t] == 0.f) continue;
    const int n = th_tensor_floats(t, D, F, Mx);
    float r = 0.f;
    for (int i = tid; i < n; i += kThThreads) r = fmaf(ht.w[t][i], ht.w[t][i], r);
    reg = fmaf(hl.l2[t], th_block_sum(r, sm.part), reg);
  }
  if (tid == 0) {
    hl.loss_out[0] = se * hl.inv_B + reg;
    *hl.counter = 0u;
  }
}

// Batch statistics of a (B, kThH1) matrix: per feature the mean and the biased variance, two passes, every sum in a
// fixed order (kThStatLanes strided partial sums, then a tree).  stat = mean | 1 / sqrt(var + eps); the moving
// statistics move towards the batch's: moving -= (moving - batch) * (1 - momentum).
__global__ __launch_bounds__(kThThreads) void th_bn_stats(const float* __restrict__ a1, float* __restrict__ stat,
                                                          float* __restrict__ moving_mean,
                                                          float* __restrict__ moving_var, float momentum, float eps,
                                                          int B) {
  __shared__ float red[kThThreads];
  const int tid = threadIdx.x, lane = tid / kThStatLanes, fl = tid % kThStatLanes;
  const int f = blockIdx.x * kThStatLanes + fl;
  auto lane_sum = [&](float v) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = kThStatLanes / 2; o > 0; o >>= 1) {
      if (lane < o) red[tid] += red[tid + o * kThStatLanes];
      __syncthreads();
    }
    return red[fl];
  };
  float s = 0.f;
  for (int b = lane; b < B; b += kThStatLanes) s += a1[(int64_t)b * kThH1 + f];
  const float mean = lane_sum(s) / (float)B;
  float q = 0.f;
  for (int b = lane; b < B; b += kThStatLanes) {
    const float d = a1[(int64_t)b * kThH1 + f] - mean;
    q = fmaf(d, d, q);
  }
  const float var = lane_sum(q) / (float)B;
  if (lane == 0) {
    stat[f] = mean;
    stat[kThH1 + f] = 1.0f / sqrtf(var + eps);
    moving_mean[f] -= (moving_mean[f] - mean) * (1.0f - momentum);
    moving_var[f] -= (moving_var[f] - var) * (1.0f - momentum);
  }
}

// Backward from the loss to the gradient of BatchNormalization's output: dz3 (B,64), dz2 (B,128), g (B,256).
// kWeighted: the prediction's gradient seed carries the sample's weight w[b] (live samples only read it); the other
// instance never looks at its last argument.
template <bool kWeighted>
__global__ __launch_bounds__(kThThreads) void th_bwd_post(ThTensors ht, const float* __restrict__ saved,
                                                          float* __restrict__ work, const float* __restrict__ y,
                                                          const float* __restrict__ dloss, int loss_kind, float delta,
                                                          int B, int F, int Mx, bool dropout, DropoutArgs drop,
                                                          const float* __restrict__ w) {
  __shared__ ThSmem sm;
  const int tid = threadIdx.x, b0 = blockIdx.x * kThSPB;
  const ThSaved so = th_saved(B, F, Mx);
  const ThWork wo = th_work(B, F, Mx);
  th_load_tile(sm.a2, kThH2, saved + so.a2, kThH2, b0, B);
  th_load_tile(sm.a3, kThH3, saved + so.a3, kThH3, b0, B);
  if (tid < kThSPB) {
    if constexpr (kWeighted)
      sm.small[tid] = b0 + tid < B ? w[b0 + tid] * th_loss_grad(loss_kind, delta, saved[so.pred + b0 + tid] - y[b0 + tid]) /
                                         (float)B * dloss[0]
                                   : 0.f;
    else
      sm.small[tid] = b0 + tid < B ? th_loss_grad(loss_kind, delta, saved[so.pred + b0 + tid] - y[b0 + tid]) / (float)B * dloss[0]
                                   : 0.f;
  }
  __syncthreads();
  if (tid < kThSPB && b0 + tid < B) work[wo.dpred + b0 + tid] = sm.small[tid];
  float* dz3 = sm.fp;  // [kThSPB][kThH3]
  for (int idx = tid; idx < kThSPB * kThH3; idx += kThThreads) {
    const int s = idx / kThH3, j = idx - s * kThH3;
    dz3[idx] = sm.a3[idx] > 0.f ? ht.w[16][j] * sm.small[s] : 0.f;
  }
  __syncthreads();
  float* dz2 = sm.x;  // [kThSPB][kThH2]
  th_dense(dz3, kThH3, kThH3, ht.w[14], 1, kThH3, nullptr, kThH2, dz2, kThH2, false, sm.part);
  {
    DropoutKey key{};
    if (dropout) key = dropout_key(drop);
    for (int idx = tid; idx < kThSPB * (kThH2 / 4); idx += kThThreads) {
      const int s = idx / (kThH2 / 4), c4 = idx - s * (kThH2 / 4);
      Philox4 p{};
      if (dropout) p = dropout_bits(key, b0 + s, c4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = s * kThH2 + 4 * c4 + q;
        float v = sm.a2[e] > 0.f ? dz2[e] : 0.f;  // (a dropped unit has a2 == 0; the regenerated mask says the same)
        if (dropout) v = dropout_apply(key, p.v[q], v);
        dz2[e] = v;
      }
    }
    __syncthreads();
  }
  th_dense(dz2, kThH2, kThH2, ht.w[12], 1, kThH2, nullptr, kThH1, sm.bn, kThH1, false, sm.part);
  th_store_tile(dz3, kThH3, work + wo.dz3, kThH3, b0, B);
  th_store_tile(dz2, kThH2, work + wo.dz2, kThH2, b0, B);
  th_store_tile(sm.bn, kThH1, work + wo.g, kThH1, b0, B);
}

// Per feature: mean_b g and mean_b g * xhat (the two sums of BatchNormalization's backward); dbeta += sum g,
// dgamma += sum g * xhat where those buffers are given, each with its l2 penalty's 2 * l2 * w * dloss as th_param_grads.
__global__ __launch_bounds__(kThThreads) void th_bn_bwd_stats(const float* __restrict__ a1,
                                                              const float* __restrict__ stat,
                                                              const float* __restrict__ g, float* __restrict__ bst,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float l2_gamma,
                                                              float l2_beta, const float* __restrict__ dloss, int B) {
  __shared__ float red[kThThreads];
  const int tid = threadIdx.x, lane = tid / kThStatLanes, fl = tid % kThStatLanes;
  const int f = blockIdx.x * kThStatLanes + fl;
  auto lane_sum = [&](float v) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = kThStatLanes / 2; o > 0; o >>= 1) {
      if (lane < o) red[tid] += red[tid + o * kThStatLanes];
      __syncthreads();
    }
    return red[fl];
  };
  const float mean = stat[f], inv_std = stat[kThH1 + f];
  float s = 0.f, q = 0.f;
  for (int b = lane; b < B; b += kThStatLanes) {
    const float gv = g[(int64_t)b * kThH1 + f];
    s += gv;
    q = fmaf(gv, (a1[(int64_t)b * kThH1 + f] - mean) * inv_std, q);
  }
  const float sg = lane_sum(s);
  const float sgx = lane_sum(q);
  if (lane == 0) {
    bst[f] = sg / (float)B;
    bst[kThH1 + f] = sgx / (float)B;
    if (dbeta) dbeta[f] += l2_beta != 0.f ? fmaf(2.0f * l2_beta * dloss[0], beta[f], sg) : sg;
    if (dgamma) dgamma[f] += l2_gamma != 0.f ? fmaf(2.0f * l2_gamma * dloss[0], gamma[f], sgx) : sgx;
  }
}

// flags of th_bwd_pre
enum { kThNeedBase = 1, kThNeedPooled = 2 };

// From g to dz1 (B,256) through BatchNormalization and the relu of mp_dense_1, then (kThNeedBase) down the base head:
// dpr (B,2,Mx), dfp (B,2,F) and (kThNeedPooled) dpooled_cat / dpooled_an (B,D).
__global__ __launch_bounds__(kThThreads) void th_bwd_pre(ThTensors ht, const float* __restrict__ saved,
                                                         float* __restrict__ work, int batch_stats, int flags,
                                                         float* __restrict__ dpc, float* __restrict__ dpa, int B,
                                                         int D, int F, int Mx) {
  __shared__ ThSmem sm;
  const int tid = threadIdx.x, b0 = blockIdx.x * kThSPB;
  const ThSaved so = th_saved(B, F, Mx);
  const ThWork wo = th_work(B, F, Mx);
  {
    const float mean = saved[so.stat + tid], inv_std = saved[so.stat + kThH1 + tid], gam = ht.w[10][tid];
    const float mg = batch_stats ? work[wo.bst + tid] : 0.f, mgx = batch_stats ? work[wo.bst + kThH1 + tid] : 0.f;
    for (int s = 0; s < kThSPB; ++s) {
      float v = 0.f;
      if (b0 + s < B) {
        const float a = saved[so.a1 + (int64_t)(b0 + s) * kThH1 + tid];
        const float gv = work[wo.g + (int64_t)(b0 + s) * kThH1 + tid];
        const float xh = (a - mean) * inv_std;
        v = a > 0.f ? gam * inv_std * (gv - mg - xh * mgx) : 0.f;
        work[wo.dz1 + (int64_t)(b0 + s) * kThH1 + tid] = v;
      }
      sm.a1[s * kThH1 + tid] = v;
    }
    __syncthreads();
  }
  if (!(flags & kThNeedBase)) return;
  th_dense(sm.a1, kThH1, kThH1, ht.w[8], 1, kThH1, nullptr, Mx, sm.mix, kHeadMaxDim, false, sm.part);  // dmix
  for (int idx = tid; idx < kThSPB * 2 * Mx; idx += kThThreads) {
    const int s = idx / (2 * Mx), r = idx - s * 2 * Mx, g = r / Mx, j = r - g * Mx;
    const bool live = b0 + s < B;
    const float v = live && saved[so.pr + (int64_t)(b0 + s) * 2 * Mx + r] > 0.f ? sm.mix[s * kHeadMaxDim + j] : 0.f;
    sm.pr[(s * 2 + g) * kHeadMaxDim + j] = v;
    if (live) work[wo.dpr + (int64_t)(b0 + s) * 2 * Mx + r] = v;
  }
  __syncthreads();
  for (int g = 0; g < 2; ++g)
    th_dense(sm.pr + g * kHeadMaxDim, 2 * kHeadMaxDim, Mx, ht.w[4 + 2 * g], 1, Mx, nullptr, F, sm.fp + g * kHeadMaxDim, 2 * kHeadMaxDim,
             false, sm.part);
  for (int idx = tid; idx < kThSPB * 2 * F; idx += kThThreads) {
    const int s = idx / (2 * F), r = idx - s * 2 * F, g = r / F, j = r - g * F;
    const bool live = b0 + s < B;
    const float v = live && saved[so.fp + (int64_t)(b0 + s) * 2 * F + r] > 0.f ? sm.fp[(s * 2 + g) * kHeadMaxDim + j] : 0.f;
    sm.fp[(s * 2 + g) * kHeadMaxDim + j] = v;
    if (live) work[wo.dfp + (int64_t)(b0 + s) * 2 * F + r] = v;
  }
  __syncthreads();
  if (!(flags & kThNeedPooled)) return;
  for (int g = 0; g < 2; ++g) {
    th_dense(sm.fp + g * kHeadMaxDim, 2 * kHeadMaxDim, F, ht.w[2 * g], 1, F, nullptr, D, sm.x, kHeadMaxX, false, sm.part);
    th_store_tile(sm.x, kHeadMaxX, g == 0 ? dpc : dpa, D, b0, B);
    __syncthreads();
  }
}

// Parameter gradients: job q adds, for every element (i, j) of its (I, J) tensor,
//   sum_b a[b * lda + i] * g[b * ldg + j]   (a null: a bias, sum_b g[b * ldg + j])   + 2 * l2 * w[i, j] * dloss
// to out[i * J + j]; one thread per element, the batch in order (no atomics).  kRows: a job with `arow` reads row
// arow[b] of its nrow-row table `a` in place of row b (an index outside the table: a row of zeros); the other instance
// never looks at arow / nrow.
constexpr int kThJobs = 16;
struct ThJobs {
  const float* a[kThJobs];
  const float* g[kThJobs];
  const float* w[kThJobs];
  float* out[kThJobs];
  int lda[kThJobs], ldg[kThJobs], I[kThJobs], J[kThJobs];
  const int* arow[kThJobs];
  int nrow[kThJobs];
  int first_block[kThJobs + 1];
  float l2[kThJobs];
  int n;
};
template <bool kRows>
__global__ __launch_bounds__(kThThreads) void th_param_grads(ThJobs jobs, const float* __restrict__ dloss, int B) {
  int q = 0;
  for (int t = 1; t < kThJobs; ++t)
    if (t < jobs.n && (int)blockIdx.x >= jobs.first_block[t]) q = t;
  const int I = jobs.I[q], J = jobs.J[q];
  const int e = ((int)blockIdx.x - jobs.first_block[q]) * kThThreads + threadIdx.x;
  if (e >= I * J) return;
  const int i = e / J, j = e - i * J;
  const float* __restrict__ a = jobs.a[q];
  const float* __restrict__ g = jobs.g[q];
  const int lda = jobs.lda[q], ldg = jobs.ldg[q];
  float acc = 0.f;
  if (kRows && a && jobs.arow[q]) {
    const int* __restrict__ ar = jobs.arow[q];
    const unsigned nrow = (unsigned)jobs.nrow[q];
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
      const int row = ar[b];
      const float av = (unsigned)row < nrow ? a[(int64_t)row * lda + i] : 0.f;
      acc = fmaf(av, g[(int64_t)b * ldg + j], acc);
    }
  } else if (a) {
#pragma unroll 4
    for (int b = 0; b < B; ++b) acc = fmaf(a[(int64_t)b * lda + i], g[(int64_t)b * ldg + j], acc);
  } else {
#pragma unroll 4
    for (int b = 0; b < B; ++b) acc += g[(int64_t)b * ldg + j];
  }
  if (jobs.l2[q] != 0.f) acc = fmaf(2.0f * jobs.l2[q] * dloss[0], jobs.w[q][e], acc);
  jobs.out[q][e] += acc;
}

int th_check_dims(const char* what, int D, int F, int Mx) {
  if (D > kHeadMaxX || F > kHeadMaxDim || Mx > kHeadMaxDim)
    return fail(IMPNN_E_UNSUPPORTED, "%s: dims D=%d (<= %d) F=%d Mx=%d (<= %d)", what, D, kHeadMaxX, F, Mx, kHeadMaxDim);
  return IMPNN_OK;
}

}  // namespace

int64_t transfer_head_saved_floats(int B, int F, int Mx) { return th_saved(B, F, Mx).total; }
int64_t transfer_head_bwd_workspace_floats(int B, int F, int Mx) { return th_work(B, F, Mx).total; }
int64_t transfer_head_loss_workspace_floats(int B) { return (B + kThSPB - 1) / kThSPB + 4; }

int launch_transfer_head(const TransferHeadCall& c) {
  if (int rc = th_check_dims("transfer_head", c.D, c.F, c.Mx)) return rc;
  ThTensors ht;
  for (int t = 0; t < kThTensors; ++t) {
    if (!c.weights[t]) return fail(IMPNN_E_BADARG, "transfer_head: null weight tensor %d", t);
    ht.w[t] = c.weights[t];
  }
  ThLoss hl{};
  if (c.y) {
    hl.y = c.y, hl.loss_out = c.loss;
    hl.counter = reinterpret_cast<unsigned int*>(c.workspace);
    hl.partial = c.workspace + 4;
    for (int t = 0; t < kThTensors; ++t) hl.l2[t] = c.l2[t];
    hl.delta = c.delta, hl.kind = c.loss_kind, hl.inv_B = 1.0f / (float)c.B;
  }
  const int groups = (c.B + kThSPB - 1) / kThSPB;
  // the launch that ends with the loss: the weighted instance where the call has weights
  // (the indexed instances where the launch holds the tile load of an indexed call; the index is null otherwise)
  const bool rows = c.cat_row != nullptr;
  auto loss_forward = [&](int flags) {
    const bool weighted = c.y && c.sample_weight;
    const bool indexed = rows && (flags & kThPre);
    const auto kernel = indexed ? (weighted ? th_forward<true, true> : th_forward<false, true>)
                                : (weighted ? th_forward<true, false> : th_forward<false, false>);
    kernel<<<groups, kThThreads, 0, c.stream>>>(c.pc, c.pa, ht, c.moving_mean, c.moving_var, c.bn_eps, flags, c.saved,
                                                c.out, c.B, c.D, c.F, c.Mx, c.dropout, c.drop, hl,
                                                weighted ? c.sample_weight : nullptr, indexed ? c.cat_row : nullptr,
                                                indexed ? c.an_row : nullptr, c.C, c.A);
  };
  const ThSaved so = th_saved(c.B, c.F, c.Mx);
  if (c.bn_batch) {
    const auto pre = rows ? th_forward<false, true> : th_forward<false, false>;
    pre<<<groups, kThThreads, 0, c.stream>>>(c.pc, c.pa, ht, c.moving_mean, c.moving_var, c.bn_eps, kThPre, c.saved,
                                             nullptr, c.B, c.D, c.F, c.Mx, false, DropoutArgs{}, ThLoss{}, nullptr,
                                             c.cat_row, c.an_row, c.C, c.A);
    if (int rc = check_launch("transfer_head (pre)")) return rc;
    th_bn_stats<<<kThH1 / kThStatLanes, kThThreads, 0, c.stream>>>(c.saved + so.a1, c.saved + so.stat, c.moving_mean,
                                                                   c.moving_var, c.bn_momentum, c.bn_eps, c.B);
    if (int rc = check_launch("transfer_head (statistics)")) return rc;
    loss_forward(kThPost | kThBatchStats);
    return check_launch("transfer_head (post)");
  }
  loss_forward(kThPre | kThPost);
  return check_launch("transfer_head");
}

int launch_transfer_head_bwd(const TransferHeadCall& c) {
  if (int rc = th_check_dims("transfer_head_bwd", c.D, c.F, c.Mx)) return rc;
  ThTensors ht;
  for (int t = 0; t < kThTensors; ++t) {
    if (!c.weights[t]) return fail(IMPNN_E_BADARG, "transfer_head_bwd: null weight tensor %d", t);
    ht.w[t] = c.weights[t];
  }
  const int B = c.B, D = c.D, F = c.F, Mx = c.Mx;
  const int groups = (B + kThSPB - 1) / kThSPB;
  const ThSaved so = th_saved(B, F, Mx);
  const ThWork wo = th_work(B, F, Mx);
  float* const* dw = c.dweights;
  const auto bwd_post = c.sample_weight ? th_bwd_post<true> : th_bwd_post<false>;
  bwd_post<<<groups, kThThreads, 0, c.stream>>>(ht, c.saved, c.workspace, c.y, c.dloss, c.loss_kind, c.delta, B, F, Mx,
                                                c.dropout, c.drop, c.sample_weight);
  if (int rc = check_launch("transfer_head_bwd (post)")) return rc;
  if (c.bn_batch) {
    th_bn_bwd_stats<<<kThH1 / kThStatLanes, kThThreads, 0, c.stream>>>(c.saved + so.a1, c.saved + so.stat,
                                                                      c.workspace + wo.g, c.workspace + wo.bst, dw[10],
                                                                      dw[11], c.weights[10], c.weights[11], c.l2[10],
                                                                      c.l2[11], c.dloss, B);
    if (int rc = check_launch("transfer_head_bwd (statistics)")) return rc;
  }
  const bool pooled = c.dpc != nullptr;
  bool base = pooled;
  for (int t = 0; t < 8; ++t) base = base || dw[t];
  th_bwd_pre<<<groups, kThThreads, 0, c.stream>>>(ht, c.saved, c.workspace, c.bn_batch ? 1 : 0,
                                                  (base ? kThNeedBase : 0) | (pooled ? kThNeedPooled : 0), c.dpc, c.dpa,
                                                  B, D, F, Mx);
  if (int rc = check_launch("transfer_head_bwd (pre)")) return rc;
  // the parameter gradients of the trainable tensors (gamma and beta left the statistics kernel; with the moving
  // statistics BatchNormalization is frozen and has none)
  ThJobs jobs{};
  int nblocks = 0;
  bool indexed = false;
  auto add = [&](int t, const float* a, int lda, const float* g, int ldg, int I, int J, const int* arow = nullptr,
                 int nrow = 0) {
    if (!dw[t]) return;
    const int q = jobs.n++;
    jobs.arow[q] = arow, jobs.nrow[q] = nrow, indexed = indexed || arow;
    jobs.a[q] = a, jobs.lda[q] = lda, jobs.g[q] = g, jobs.ldg[q] = ldg, jobs.I[q] = I, jobs.J[q] = J;
    jobs.w[q] = c.weights[t], jobs.out[q] = dw[t], jobs.l2[q] = c.l2[t];
    jobs.first_block[q] = nblocks;
    nblocks += (I * J + kThThreads - 1) / kThThreads;
  };
  const float* sv = c.saved;
  const float* wk = c.workspace;
  for (int g = 0; g < 2; ++g) {
    add(2 * g, g == 0 ? c.pc : c.pa, D, wk + wo.dfp + g * F, 2 * F, D, F, g == 0 ? c.cat_row : c.an_row,
        g == 0 ? c.C : c.A);
    add(2 * g + 1, nullptr, 0, wk + wo.dfp + g * F, 2 * F, 1, F);
    add(4 + 2 * g, sv + so.fp + g * F, 2 * F, wk + wo.dpr + g * Mx, 2 * Mx, F, Mx);
    add(5 + 2 * g, nullptr, 0, wk + wo.dpr + g * Mx, 2 * Mx, 1, Mx);
  }
  add(8, sv + so.mix, Mx, wk + wo.dz1, kThH1, Mx, kThH1);
  add(9, nullptr, 0, wk + wo.dz1, kThH1, 1, kThH1);
  add(12, sv + so.bn, kThH1, wk + wo.dz2, kThH2, kThH1, kThH2);
  add(13, nullptr, 0, wk + wo.dz2, kThH2, 1, kThH2);
  add(14, sv + so.a2, kThH2, wk + wo.dz3, kThH3, kThH2, kThH3);
  add(15, nullptr, 0, wk + wo.dz3, kThH3, 1, kThH3);
  add(16, sv + so.a3, kThH3, wk + wo.dpred, 1, kThH3, 1);
  add(17, nullptr, 0, wk + wo.dpred, 1, 1, 1);
  jobs.first_block[jobs.n] = nblocks;
  if (jobs.n == 0) return IMPNN_OK;
  const auto param_grads = indexed ? th_param_grads<true> : th_param_grads<false>;
  param_grads<<<nblocks, kThThreads, 0, c.stream>>>(jobs, c.dloss, B);
  return check_launch("transfer_head_bwd (parameters)");
}

}  // namespace impnn
