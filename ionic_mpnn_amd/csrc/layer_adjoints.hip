// The small adjoints of the layer-at-a-time path: what Keras autodiff does for the reference's
// embedding lookups (a1/a2), Reduce (a5, models/layers.py:57-83) and GlobalSumPooling (a8, models/layers.py:161-164).
// Each is the adjoint of its forward in layer_kernels.hip with the same masks (tgt > 0, atom_ids > 0) and the same
// "out-of-range index == padding" rule.  Written for any D (VALU, f32).  The Reduce and pool adjoints write every
// output element once: no sum, the same bits on every run.  The embedding adjoint adds with float atomics, so rows of
// one id meet in any order (embed_rows.hip has the fixed-order form for listed rows).
#include "kernel_device.h"

namespace impnn {
namespace {

// ---------------------------------------------------------------------------------------
// a1/a2 backward: dtable[ids[r], :] += dout[r, :]   (float atomics: rows of one id meet in any order).
// Vocabularies are small (~10^2 rows), so thousands of rows collide on the same table row: when the table
// fits LDS every workgroup first sums its rows there (LDS atomics) and touches HBM once per entry.
// ---------------------------------------------------------------------------------------
__global__ void embed_gather_bwd_kernel(const int32_t* __restrict__ ids, const float* __restrict__ dout,
                                        float* __restrict__ dtable, int64_t rows, int vocab, int dim, int use_lds) {
  extern __shared__ __align__(16) float smem[];
  const int64_t total = rows * dim;
  if (use_lds) {
    const int tsize = vocab * dim;
    for (int t = threadIdx.x; t < tsize; t += blockDim.x) smem[t] = 0.f;
    __syncthreads();
    // contiguous slice of rows per workgroup
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < total ? lo + per : total;
    constexpr int kU = 8;  // independent (id, value) loads in flight per thread
    for (int64_t t0 = lo + threadIdx.x; t0 < hi; t0 += (int64_t)kU * blockDim.x) {
      float v[kU];
      int at[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t t = t0 + (int64_t)u * blockDim.x;
        at[u] = -1;
        v[u] = 0.f;
        if (t < hi) {
          const int64_t r = t / dim;
          const int id = ids[r];
          v[u] = dout[t];
          if ((unsigned)id < (unsigned)vocab) at[u] = id * dim + (int)(t - r * dim);
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u)
        if (at[u] >= 0 && v[u] != 0.f) atomicAdd(&smem[at[u]], v[u]);  // (padding atoms: half of the rows, all zeros)
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tsize; t += blockDim.x) {
      const float v = smem[t];
      if (v != 0.f) atomicAdd(&dtable[t], v);
    }
    return;
  }
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / dim;
    const int c = (int)(t - r * dim);
    const int id = ids[r];
    if ((unsigned)id < (unsigned)vocab) atomicAdd(&dtable[(int64_t)id * dim + c], dout[t]);
  }
}

// ---------------------------------------------------------------------------------------
// a5 backward (models/layers.py:57-83): dmessages[b,e,:] = tgt > 0 ? dagg[b,tgt,:] : 0
// ---------------------------------------------------------------------------------------
__global__ void reduce_scatter_bwd_kernel(const float* __restrict__ dagg, const int32_t* __restrict__ tgt,
                                          int tgt_stride, float* __restrict__ dm, int64_t BE, int N, int E, int D) {
  const int64_t total = BE * D;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t be = t / D;
    const int c = (int)(t - be * D);
    const int64_t b = be / E;
    const int tg = tgt[be * tgt_stride];
    dm[t] = (tg > 0 && tg < N) ? dagg[(b * N + tg) * D + c] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// a8 backward (models/layers.py:161-164): dh[b,n,:] = atom_ids[b,n] > 0 ? dpooled[b,:] : 0
// ---------------------------------------------------------------------------------------
__global__ void global_sum_pool_bwd_kernel(const float* __restrict__ dp, const int32_t* __restrict__ ids,
                                           float* __restrict__ dh, int64_t BN, int N, int D) {
  const int64_t total = BN * D;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bn = t / D;
    const int c = (int)(t - bn * D);
    dh[t] = ids[bn] > 0 ? dp[(bn / N) * D + c] : 0.f;
  }
}

}  // namespace

int launch_embed_gather_bwd(const int32_t* ids, const float* dout, float* dtable, int64_t rows, int vocab, int dim,
                            hipStream_t s) {
  const size_t lds = sizeof(float) * (size_t)vocab * dim;
  const int use_lds = lds <= 64 * 1024 && rows * dim >= 8 * (int64_t)vocab * dim;
  if (use_lds && lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)embed_gather_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  embed_gather_bwd_kernel<<<grid_for(rows * dim, use_lds ? 512 : 256 * 8), kBlock, use_lds ? lds : 0, s>>>(
      ids, dout, dtable, rows, vocab, dim, use_lds);
  return check_launch("embed_gather_bwd");
}

int launch_reduce_scatter_bwd(const float* dagg, const int32_t* tgt, int tgt_stride, float* dm, int B, int N, int E,
                              int D, hipStream_t s) {
  reduce_scatter_bwd_kernel<<<grid_for((int64_t)B * E * D), kBlock, 0, s>>>(dagg, tgt, tgt_stride, dm,
                                                                              (int64_t)B * E, N, E, D);
  return check_launch("reduce_scatter_bwd");
}

int launch_global_sum_pool_bwd(const float* dp, const int32_t* ids, float* dh, int B, int N, int D, hipStream_t s) {
  global_sum_pool_bwd_kernel<<<grid_for((int64_t)B * N * D), kBlock, 0, s>>>(dp, ids, dh, (int64_t)B * N, N, D);
  return check_launch("global_sum_pool_bwd");
}

}  // namespace impnn
