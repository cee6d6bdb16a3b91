// Backward kernels of the layer-at-a-time path and the optimizer step: what Keras
// autodiff + Adam(1e-3, clipnorm=1.0) do for the reference's model.fit (train_viscosity.py:227-230,
// 328-338; train_melting_point.py:205-208).  One kernel per reference layer, the adjoint of the forward
// in layer_kernels.hip with the same masks (models/layers.py:114-115, :70 tgt > 0) and the same
// "out-of-range index == padding" rule.  Written for any D (VALU, f32); the parameter-gradient sums run
// over per-workgroup partial buffers that a second kernel adds in a fixed order, except where noted.
// Holds the embedding, pool and Reduce adjoints, the bond-table gradient, the GatedUpdate backward and Adam; the message
// adjoint (a4) and its edge sort are in message_typed.hip, the model head's backward in model_head.hip.
#include "kernel_device.h"

namespace impnn {
namespace {

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

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

__global__ void zero_floats_kernel(float* __restrict__ p, int64_t n) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) p[t] = 0.f;
}

// ---------------------------------------------------------------------------------------
// schedule A backward: A[v] = sum_k Tb[v,k] W[k]  =>  dW[k] = sum_v Tb[v,k] dA[v];  dTb[v,k] = <dA[v], W[k]>
// ---------------------------------------------------------------------------------------
__global__ void bond_type_matrices_bwd_w_kernel(const float* __restrict__ tb, const float* __restrict__ dA,
                                                float* __restrict__ dW, int Vb, int K, int DD, int accumulate) {
  const int k = blockIdx.y;
  for (int ij = blockIdx.x * blockDim.x + threadIdx.x; ij < DD; ij += gridDim.x * blockDim.x) {
    float acc = 0.f;
    int v = 0;
    for (; v + 16 <= Vb; v += 16) {  // 16 independent rows in flight; the adds stay in vocabulary order
      float x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = dA[(int64_t)(v + u) * DD + ij];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = fmaf(tb[(int64_t)(v + u) * K + k], x[u], acc);
    }
    for (; v < Vb; ++v) acc = fmaf(tb[(int64_t)v * K + k], dA[(int64_t)v * DD + ij], acc);
    dW[(int64_t)k * DD + ij] = accumulate ? dW[(int64_t)k * DD + ij] + acc : acc;
  }
}
__global__ void bond_type_matrices_bwd_t_kernel(const float* __restrict__ W, const float* __restrict__ dA,
                                                float* __restrict__ dtb, int Vb, int K, int DD, int accumulate) {
  // one wave per (v,k)
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= Vb * K) return;
  const int v = wave / K, k = wave - v * K;
  float acc = 0.f;
  const float* da = dA + (int64_t)v * DD;
  const float* w = W + (int64_t)k * DD;
  int ij = lane;
  for (; ij + 7 * 64 < DD; ij += 8 * 64) {  // 16 independent loads in flight per lane
    float x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x[u] = da[ij + 64 * u];
      y[u] = w[ij + 64 * u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(x[u], y[u], acc);
  }
  for (; ij < DD; ij += 64) acc = fmaf(da[ij], w[ij], acc);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) dtb[(int64_t)v * K + k] = accumulate ? dtb[(int64_t)v * K + k] + acc : acc;
}

// ---------------------------------------------------------------------------------------
// The same for ALL message layers of a model in one launch each (training at the reference's batch 32 is bound by
// the number of launches, and these depend on the weights only): problem p = (ion, step) has its own W_p, the bond
// embedding table is shared, so dTb sums over the problems.
// ---------------------------------------------------------------------------------------
constexpr int kBtmMax = 16;
struct BtmBatch {
  const float* W[kBtmMax];
  const float* dA[kBtmMax];
  float* out[kBtmMax];  // forward: A_p (Vb x DD); backward: dW_p (K x DD)
  int n;
};
// kernel-argument tables are indexed with constants only (a dynamic index is a dependent kernarg load per use)
#define BTM_STAGE(bt)                                                       \
  __shared__ const float* sW[kBtmMax];                                      \
  __shared__ const float* sdA[kBtmMax];                                     \
  __shared__ float* sout[kBtmMax];                                          \
  _Pragma("unroll") for (int q = 0; q < kBtmMax; ++q) if ((int)threadIdx.x == q) {  \
    sW[q] = bt.W[q];                                                        \
    sdA[q] = bt.dA[q];                                                      \
    sout[q] = bt.out[q];                                                    \
  }                                                                         \
  __syncthreads();

__global__ void bond_type_matrices_multi_kernel(const float* __restrict__ tb, BtmBatch bt, int Vb, int K, int DD) {
  BTM_STAGE(bt)
  const int v = blockIdx.y;
  const float* W = sW[blockIdx.z];
  float* out = sout[blockIdx.z];
  for (int ij = blockIdx.x * blockDim.x + threadIdx.x; ij < DD; ij += gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(tb[(int64_t)v * K + k], W[(int64_t)k * DD + ij], acc);  // as the single kernel
    out[(int64_t)v * DD + ij] = acc;
  }
}
// bond_dim <= 8 (the reference's 8): the K values W[k][ij] of a thread's element stay in registers while it walks the
// bond types, so W is read once instead of once per type (at atom_dim 128: 6 MB instead of 436 MB of L2 reads over the
// 12 layers; 86 -> ~15 us).  Same fmaf chain per output element as the kernel above: identical bits.
constexpr int kBtmSmallK = 8;
constexpr int kBtmTbMax = 4096;  // bond_table floats staged in LDS (Vb * K)
__global__ __launch_bounds__(kBlock) void bond_type_matrices_multi_smallk_kernel(const float* __restrict__ tb, BtmBatch bt,
                                                                                 int Vb, int K, int DD) {
  BTM_STAGE(bt)
  __shared__ float tb_s[kBtmTbMax];
  for (int t = threadIdx.x; t < Vb * K; t += kBlock) tb_s[t] = tb[t];
  __syncthreads();
  const float* W = sW[blockIdx.y];
  float* out = sout[blockIdx.y];
  const int ij = blockIdx.x * kBlock + threadIdx.x;
  if (ij >= DD) return;
  float w[kBtmSmallK];
#pragma unroll
  for (int k = 0; k < kBtmSmallK; ++k) w[k] = k < K ? W[(int64_t)k * DD + ij] : 0.f;
  for (int v = 0; v < Vb; ++v) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kBtmSmallK; ++k)
      if (k < K) acc = fmaf(tb_s[v * K + k], w[k], acc);
    out[(int64_t)v * DD + ij] = acc;
  }
}

__global__ void bond_type_matrices_multi_bwd_w_kernel(const float* __restrict__ tb, BtmBatch bt, int Vb, int K, int DD,
                                                      int accumulate) {
  BTM_STAGE(bt)
  const int k = blockIdx.y;
  const float* dA = sdA[blockIdx.z];
  float* dW = sout[blockIdx.z];
  for (int ij = blockIdx.x * blockDim.x + threadIdx.x; ij < DD; ij += gridDim.x * blockDim.x) {
    float acc = 0.f;
    int v = 0;
    for (; v + 16 <= Vb; v += 16) {
      float x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) x[u] = dA[(int64_t)(v + u) * DD + ij];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = fmaf(tb[(int64_t)(v + u) * K + k], x[u], acc);
    }
    for (; v < Vb; ++v) acc = fmaf(tb[(int64_t)v * K + k], dA[(int64_t)v * DD + ij], acc);
    dW[(int64_t)k * DD + ij] = accumulate ? dW[(int64_t)k * DD + ij] + acc : acc;
  }
}
__global__ void bond_type_matrices_multi_bwd_t_kernel(BtmBatch bt, float* __restrict__ dtb, int Vb, int K, int DD,
                                                      int accumulate) {
  BTM_STAGE(bt)
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= Vb * K) return;
  const int v = wave / K, k = wave - v * K;
  float acc = 0.f;
  for (int p = 0; p < bt.n; ++p) {  // problems in order, then the lanes: a fixed summation order
    const float* da = sdA[p] + (int64_t)v * DD;
    const float* w = sW[p] + (int64_t)k * DD;
    int ij = lane;
    for (; ij + 7 * 64 < DD; ij += 8 * 64) {
      float x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x[u] = da[ij + 64 * u];
        y[u] = w[ij + 64 * u];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fmaf(x[u], y[u], acc);
    }
    for (; ij < DD; ij += 64) acc = fmaf(da[ij], w[ij], acc);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) dtb[(int64_t)v * K + k] = accumulate ? dtb[(int64_t)v * K + k] + acc : acc;
}


// ---------------------------------------------------------------------------------------
// dtb[v,k] = sum_p sum_ij dA_p[v,ij] W_p[k,ij] on the matrix cores (exact f32 products): bond types on M (VT tiles of
// 16), k on N (K <= 16, padded with zeros), the contraction over (p, ij) cut into chunks of kBtC per WAVE - a lane loads
// 16 bytes of a dA row and of a W row per 16 contraction indices (the MFMA's k = the lane's quarter q, component r of
// the quad: any bijection serves as long as both operands use it).  The per-wave partials land in `part`
// ([wave][v][k]) and bond_type_matrices_t_sum_kernel adds them in wave order: bitwise reproducible.
// The one-wave-per-output kernel above walked 12 x 16 K products per lane with eight loads in flight: 116-170 us at
// atom_dim 128 - alone on the stream at the end of every backward pass, so all of it on the critical path of a step.
// ---------------------------------------------------------------------------------------
constexpr int kBtC = 256;
template <int VT>
__global__ __launch_bounds__(256) void bond_type_matrices_multi_bwd_t_mfma_kernel(BtmBatch bt, float* __restrict__ part,
                                                                                  int Vb, int K, int DD, int waves) {
  BTM_STAGE(bt)
  const int w = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63, a = lane & 15, q = lane >> 4;
  if (w >= waves) return;
  const int cpp = DD / kBtC, p = w / cpp, c0 = (w - p * cpp) * kBtC + 4 * q;
  const float* Wp = sW[p] + (int64_t)(a < K ? a : 0) * DD + c0;
  const float* dAp = sdA[p] + c0;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  f32x4_t acc[VT];
#pragma unroll
  for (int t = 0; t < VT; ++t) acc[t] = zero;
#pragma unroll 2
  for (int st = 0; st < kBtC / 16; ++st) {
    const f32x4_t wv = a < K ? ldv4(Wp + 16 * st) : zero;
    f32x4_t x[VT];
#pragma unroll
    for (int t = 0; t < VT; ++t) {
      const int v = 16 * t + a;
      x[t] = v < Vb ? ldv4(dAp + (int64_t)v * DD + 16 * st) : zero;
    }
#pragma unroll
    for (int t = 0; t < VT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t] = mfma_f32(x[t][r], wv[r], acc[t]);
  }
  float* mine = part + (int64_t)w * Vb * K;
#pragma unroll
  for (int t = 0; t < VT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int v = 16 * t + 4 * q + g;
      if (v < Vb && a < K) mine[v * K + a] = acc[t][g];
    }
}
__global__ void bond_type_matrices_t_sum_kernel(const float* __restrict__ part, float* __restrict__ dtb, int VK, int waves,
                                                int accumulate) {
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (e >= VK) return;
  float acc = 0.f;
  for (int w = lane; w < waves; w += 64) acc += part[(int64_t)w * VK + e];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) dtb[e] = accumulate ? dtb[e] + acc : acc;
}

// ---------------------------------------------------------------------------------------
// a7 backward (models/layers.py:142-156).  Forward per row, c = [h|agg]:
//   z = sig(c Wz + bz); r = sig(c Wr + br); t = tanh([r*h|agg] Wh + bh); n = (1-z) h + z t;
//   x = (n - mean) * inv; out = gamma x + beta + h
// Three launches:
//   1. gated_update_bwd_kernel: tiles of R = kBlock/D rows, intermediates recomputed from (h, agg) ->
//      dh, dagg, the pre-activation gradients dpre = [dzp|drp|dtp] (rows x 3D), r*h (rows x D), and per
//      workgroup the column sums that give dbz, dbr, dbh, dgamma, dbeta (5D floats);
//   2. tn_gemm_splitk_kernel: the three kernel gradients dW_g = in_g^T dpre_g (in_z = in_r = [h|agg],
//      in_h = [r*h|agg]) as split-K GEMMs over row chunks (64x32 output tiles, 4x2 per thread);
//   3. gated_update_reduce_kernel: adds the per-workgroup / per-chunk partials in a fixed order into dparams
//      (Wz 2D*D | bz | Wr | br | Wh | bh | gamma | beta): parameter gradients are bitwise reproducible.
// ---------------------------------------------------------------------------------------
// WLDS: the three gate kernels staged in LDS (row stride D+1: both access directions conflict-free).
// BS: workgroup size = rows per tile x D; large D uses 1024 threads so that one pass over the (L2-resident)
// kernels serves 4x more rows.
// Drop (empty, or one DropoutArgs; common.h): the dropout form - dout is read through the forward's mask and scale.
template <bool WLDS, int BS, class... Drop>
__global__ __launch_bounds__(BS) void gated_update_bwd_kernel(
    const float* __restrict__ h, const float* __restrict__ agg, const float* __restrict__ Wz,
    const float* __restrict__ bz, const float* __restrict__ Wr, const float* __restrict__ br,
    const float* __restrict__ Wh, const float* __restrict__ bh, const float* __restrict__ gamma, float eps,
    const float* __restrict__ dout, float* __restrict__ dh, float* __restrict__ dagg, float* __restrict__ dpre,
    float* __restrict__ rh_out, float* __restrict__ small, const float* __restrict__ WT, int64_t rows, int D, int R,
    Drop... drop) {
  constexpr bool kDrop = sizeof...(Drop) > 0;
  extern __shared__ __align__(16) float smem[];
  float* hs = smem;            // R*D each
  float* as = hs + R * D;
  float* zs = as + R * D;
  float* rs = zs + R * D;
  float* rhs = rs + R * D;     // r * h
  float* ts = rhs + R * D;     // tanh
  float* xs = ts + R * D;      // n, then x-hat, then dh so far
  float* g1 = xs + R * D;      // dx-hat, then dzp
  float* g2 = g1 + R * D;      // dx-hat * x-hat, then drp
  float* g3 = g2 + R * D;      // dtp
  float* st = g3 + R * D;      // 4*R: mean, inv, m1, m2
  const int LD = D + 1;
  float* wz_s = st + 4 * R;    // 2D*LD each (WLDS only)
  float* wr_s = wz_s + 2 * D * LD;
  float* wh_s = wr_s + 2 * D * LD;
  const int tid = threadIdx.x;
#define WZ(r_, c_) (WLDS ? wz_s[(r_) * LD + (c_)] : Wz[(int64_t)(r_) * D + (c_)])
#define WR(r_, c_) (WLDS ? wr_s[(r_) * LD + (c_)] : Wr[(int64_t)(r_) * D + (c_)])
#define WH(r_, c_) (WLDS ? wh_s[(r_) * LD + (c_)] : Wh[(int64_t)(r_) * D + (c_)])
  // element (r_, c_) for loops whose LANES walk r_: from LDS (padded stride) or from the transposed copies
  // WT = [Wz^T | Wr^T | Wh^T], each D x 2D, so that consecutive lanes read consecutive addresses
  const int D2 = 2 * D;
#define WZ_T(r_, c_) (WLDS ? wz_s[(r_) * LD + (c_)] : WT[(int64_t)(c_) * D2 + (r_)])
#define WR_T(r_, c_) (WLDS ? wr_s[(r_) * LD + (c_)] : WT[(int64_t)D * D2 + (int64_t)(c_) * D2 + (r_)])
#define WH_T(r_, c_) (WLDS ? wh_s[(r_) * LD + (c_)] : WT[(int64_t)2 * D * D2 + (int64_t)(c_) * D2 + (r_)])
  float s_bz = 0.f, s_br = 0.f, s_bh = 0.f, s_dg = 0.f, s_db = 0.f;  // this thread's (row slot, column) sums
  if (WLDS) {
    for (int t = threadIdx.x; t < 2 * D * D; t += BS) {
      const int rw = t / D, c = t - rw * D;
      wz_s[rw * LD + c] = Wz[t];
      wr_s[rw * LD + c] = Wr[t];
      wh_s[rw * LD + c] = Wh[t];
    }
  }
  [[maybe_unused]] DropoutKey dk{};
  if constexpr (kDrop) dk = dropout_key(dropout_of(drop...));
  const int64_t ntile = (rows + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t row0 = tile * R;
    const int nr = (int)((rows - row0) < R ? (rows - row0) : R);
    __syncthreads();
    for (int t = tid; t < nr * D; t += BS) {
      hs[t] = h[row0 * D + t];
      as[t] = agg[row0 * D + t];
    }
    __syncthreads();
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D, i = t - r * D;
      float az = bz[i], ar = br[i];
      for (int j = 0; j < D; ++j) {
        const float x = hs[r * D + j];
        az = fmaf(x, WZ(j, i), az);
        ar = fmaf(x, WR(j, i), ar);
      }
      for (int j = 0; j < D; ++j) {
        const float x = as[r * D + j];
        az = fmaf(x, WZ(D + j, i), az);
        ar = fmaf(x, WR(D + j, i), ar);
      }
      const float z = sigmoid_exact(az), rr = sigmoid_exact(ar);
      zs[t] = z;
      rs[t] = rr;
      const float rhv = rr * hs[t];
      rhs[t] = rhv;
      rh_out[row0 * D + t] = rhv;
    }
    __syncthreads();
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D, i = t - r * D;
      float ah = bh[i];
      for (int j = 0; j < D; ++j) ah = fmaf(rhs[r * D + j], WH(j, i), ah);
      for (int j = 0; j < D; ++j) ah = fmaf(as[r * D + j], WH(D + j, i), ah);
      const float tt = tanhf(ah);
      ts[t] = tt;
      xs[t] = (1.0f - zs[t]) * hs[t] + zs[t] * tt;
    }
    __syncthreads();
    for (int r = tid; r < nr; r += BS) {
      float mean = 0.f;
      for (int j = 0; j < D; ++j) mean += xs[r * D + j];
      mean /= (float)D;
      float var = 0.f;
      for (int j = 0; j < D; ++j) {
        const float d = xs[r * D + j] - mean;
        var = fmaf(d, d, var);
      }
      st[4 * r] = mean;
      st[4 * r + 1] = 1.0f / sqrtf(var / (float)D + eps);
    }
    __syncthreads();
    if constexpr (kDrop) {  // one Philox call per (row, column quad); the masked dout waits in g3 (dtp's slot)
      const int Q = (D + 3) / 4;
      for (int t4 = tid; t4 < nr * Q; t4 += BS) {
        const int r = t4 / Q, c4 = t4 - r * Q;
        const Philox4 bits = dropout_bits(dk, row0 + r, c4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 4 * c4 + u, t = r * D + i;
          if (i < D) {
            const float xh = (xs[t] - st[4 * r]) * st[4 * r + 1];
            xs[t] = xh;
            const float dy = dropout_apply(dk, bits.v[u], dout[row0 * D + t]);
            g3[t] = dy;
            const float dxh = dy * gamma[i];
            g1[t] = dxh;
            g2[t] = dxh * xh;
          }
        }
      }
    } else {
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D, i = t - r * D;
      const float xh = (xs[t] - st[4 * r]) * st[4 * r + 1];
      xs[t] = xh;
      const float dy = dout[row0 * D + t];
      const float dxh = dy * gamma[i];
      g1[t] = dxh;
      g2[t] = dxh * xh;
    }
    }
    __syncthreads();
    for (int r = tid; r < nr; r += BS) {
      float m1 = 0.f, m2 = 0.f;
      for (int j = 0; j < D; ++j) {
        m1 += g1[r * D + j];
        m2 += g2[r * D + j];
      }
      st[4 * r + 2] = m1 / (float)D;
      st[4 * r + 3] = m2 / (float)D;
    }
    __syncthreads();
    // dn -> (dzp, dtp), first part of dh; column sums for dgamma / dbeta
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D;
      const float dy = kDrop ? g3[t] : dout[row0 * D + t];
      const float xh = xs[t];
      const float dn = st[4 * r + 1] * (g1[t] - st[4 * r + 2] - xh * st[4 * r + 3]);
      const float z = zs[t], tt = ts[t];
      const float dzp = dn * (tt - hs[t]) * z * (1.0f - z);
      const float dtp = dn * z * (1.0f - tt * tt);
      g1[t] = dzp;
      g3[t] = dtp;
      xs[t] = dy + dn * (1.0f - z);  // dh so far (x-hat is dead)
      if (t == tid) {                 // BS == R*D: one element per thread, fixed (slot, column)
        s_dg = fmaf(dy, xh, s_dg);
        s_db += dy;
        s_bz += dzp;
        s_bh += dtp;
      }
    }
    __syncthreads();
    // dc2 = dtp Wh^T: lower half -> through r*h, upper half -> dagg
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D, i = t - r * D;
      float lo = 0.f, hi = 0.f;
      for (int j = 0; j < D; ++j) {
        const float d = g3[r * D + j];
        lo = fmaf(d, WH_T(i, j), lo);
        hi = fmaf(d, WH_T(D + i, j), hi);
      }
      const float rr = rs[t];
      const float drp = lo * hs[t] * rr * (1.0f - rr);
      g2[t] = drp;
      xs[t] += lo * rr;
      zs[t] = hi;  // dagg so far (z is dead)
      if (t == tid) s_br += drp;
    }
    __syncthreads();
    // dc = dzp Wz^T + drp Wr^T; dpre leaves for the kernel-gradient GEMMs
    for (int t = tid; t < nr * D; t += BS) {
      const int r = t / D, i = t - r * D;
      float lo = 0.f, hi = 0.f;
      for (int j = 0; j < D; ++j) {
        const float dz = g1[r * D + j], dr = g2[r * D + j];
        lo = fmaf(dz, WZ_T(i, j), lo);
        lo = fmaf(dr, WR_T(i, j), lo);
        hi = fmaf(dz, WZ_T(D + i, j), hi);
        hi = fmaf(dr, WR_T(D + i, j), hi);
      }
      dh[row0 * D + t] = xs[t] + lo;
      dagg[row0 * D + t] = zs[t] + hi;
      float* dp = dpre + (row0 + r) * 3 * D;
      dp[i] = g1[t];
      dp[D + i] = g2[t];
      dp[2 * D + i] = g3[t];
    }
  }
  // column sums: thread tid holds (slot tid / D, column tid % D); add the slots in a fixed order
  __syncthreads();
  float* red = smem;  // 5 * BS
  red[tid] = s_bz;
  red[BS + tid] = s_br;
  red[2 * BS + tid] = s_bh;
  red[3 * BS + tid] = s_dg;
  red[4 * BS + tid] = s_db;
  __syncthreads();
  float* mine = small + (int64_t)blockIdx.x * 5 * D;
  for (int q = tid; q < 5 * D; q += BS) {
    const int which = q / D, i = q - which * D;
    float acc = 0.f;
    for (int slot = 0; slot < R; ++slot) acc += red[which * BS + slot * D + i];
    mine[q] = acc;
  }
}
#undef WZ
#undef WR
#undef WH
#undef WZ_T
#undef WR_T
#undef WH_T

// ---------------------------------------------------------------------------------------
// a7 backward for D = 32 on the matrix cores (exact f32 products, v_mfma_f32_16x16x4_f32), the adjoint of
// gated_update_d32_kernel in layer_kernels.hip with the same layout: 16 rows per wave and iteration, rows on the
// MFMA N dimension (lane & 15), features on M, so every accumulator tile (feature 4*(lane>>4)+reg) is directly the
// B operand of the next product.  The gate kernels sit in LDS twice: transposed ((gate, out) rows of 2D inputs,
// stride 68) for the forward recompute, and as stored ((gate, in) rows of D outputs, stride 36) for the products
// with the pre-activation gradients.  Outputs and partial sums are those of gated_update_bwd_kernel.
// ---------------------------------------------------------------------------------------
// (row16_sum_f sums over the 16 lanes of a DPP row: here the rows of one feature quarter)
constexpr int kBwT = 68;  // stride of the transposed kernels (rows: gate*32 + out, cols: 2D inputs)
constexpr int kBwN = 36;  // stride of the natural kernels (rows: gate*64 + in, cols: D outputs)

// SAVED: dpre / rh_out arrive holding the training forward's z, r, tanh(t) / r * h (gated_update_d32_kernel's `save`):
// no recompute, no transposed kernels in LDS - 24 of the kernel's 48 MFMAs per 16 rows.
// Drop: as gated_update_bwd_kernel.
template <bool SAVED, class... Drop>
__global__ __launch_bounds__(kBlock, SAVED ? 2 : 1) void gated_update_bwd_d32_kernel(
    const float* __restrict__ h, const float* __restrict__ agg, const float* __restrict__ Wz,
    const float* __restrict__ bz, const float* __restrict__ Wr, const float* __restrict__ br,
    const float* __restrict__ Wh, const float* __restrict__ bh, const float* __restrict__ gamma, float eps,
    const float* __restrict__ dout, float* __restrict__ dh, float* __restrict__ dagg, float* __restrict__ dpre,
    float* __restrict__ rh_out, float* __restrict__ small, int64_t rows, Drop... drop) {
  constexpr int D = 32;
  extern __shared__ __align__(16) float smem[];
  float* wt = smem;                       // 3*D rows x kBwT (not with SAVED)
  float* wn = wt + (SAVED ? 0 : 3 * D * kBwT);  // 3*2D rows x kBwN
  float* wvec = wn + 3 * 2 * D * kBwN;    // bz | br | bh | gamma
  float* red = wvec + 4 * D;              // 4 waves x 5 x D column sums
  for (int t = threadIdx.x; t < 3 * 2 * D * D; t += kBlock) {
    const int gate = t / (2 * D * D), rem = t - gate * 2 * D * D;
    const int jj = rem / D, io = rem - jj * D;  // keras kernel (in = jj, out = io)
    const float* Wg = gate == 0 ? Wz : (gate == 1 ? Wr : Wh);
    const float w = Wg[rem];
    if (!SAVED) wt[(gate * D + io) * kBwT + jj] = w;
    wn[(gate * 2 * D + jj) * kBwN + io] = w;
  }
  for (int t = threadIdx.x; t < 4 * D; t += kBlock) {
    const int v = t / D, i = t - v * D;
    wvec[t] = (v == 0 ? bz : v == 1 ? br : v == 2 ? bh : gamma)[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = lane & 15, q = lane >> 4;
  const int64_t ntiles = (rows + 15) >> 4;
  const int64_t wave_id = (int64_t)blockIdx.x * (kBlock >> 6) + wave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock >> 6);
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4_t s_bz[2] = {zero4, zero4}, s_br[2] = {zero4, zero4}, s_bh[2] = {zero4, zero4};
  f32x4_t s_dg[2] = {zero4, zero4}, s_db[2] = {zero4, zero4};
  const f32x4_t gm0 = ldv4(wvec + 3 * D + 4 * q), gm1 = ldv4(wvec + 3 * D + 16 + 4 * q);
  [[maybe_unused]] DropoutKey dk{};
  if constexpr (sizeof...(Drop) > 0) dk = dropout_key(dropout_of(drop...));
  for (int64_t tile = wave_id; tile < ntiles; tile += nwaves) {
    const int64_t row = tile * 16 + a;
    const bool live = row < rows;
    const int64_t rl = live ? row : rows - 1;  // clamped load address; stores and sums are masked through dy = 0
    [[maybe_unused]] uint32_t keep = 0;  // dropout: the forward's keep bits of columns 4q + i (bit i), 16 + 4q + i (4 + i)
    if constexpr (sizeof...(Drop) > 0) {
      const Philox4 m0 = dropout_bits(dk, rl, q), m1 = dropout_bits(dk, rl, 4 + q);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        keep |= (uint32_t)((m0.v[i] >> 8) >= dk.thr) << i | (uint32_t)((m1.v[i] >> 8) >= dk.thr) << (4 + i);
    }
    const f32x4_t h0 = ldv4(h + rl * D + 4 * q), h1 = ldv4(h + rl * D + 16 + 4 * q);
    const f32x4_t a0 = ldv4(agg + rl * D + 4 * q), a1 = ldv4(agg + rl * D + 16 + 4 * q);
    f32x4_t dy0 = ldv4(dout + rl * D + 4 * q), dy1 = ldv4(dout + rl * D + 16 + 4 * q);
    if (!live) {
      dy0 = zero4;
      dy1 = zero4;
    }
    if constexpr (sizeof...(Drop) > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dy0[i] = (keep >> i) & 1u ? dy0[i] * dk.scale : 0.0f;
        dy1[i] = (keep >> (4 + i)) & 1u ? dy1[i] * dk.scale : 0.0f;
      }
    }
    // ---- forward recompute (as gated_update_d32_kernel), or what that kernel kept
    f32x4_t z0, z1, r0, r1, t0, t1;
    if constexpr (SAVED) {
      const float* sv = dpre + rl * 3 * D + 4 * q;
      z0 = ldv4(sv); z1 = ldv4(sv + 16);
      r0 = ldv4(sv + D); r1 = ldv4(sv + D + 16);
      t0 = ldv4(sv + 2 * D); t1 = ldv4(sv + 2 * D + 16);
    } else {
    z0 = ldv4(wvec + 4 * q); z1 = ldv4(wvec + 16 + 4 * q);
    r0 = ldv4(wvec + D + 4 * q); r1 = ldv4(wvec + D + 16 + 4 * q);
    t0 = ldv4(wvec + 2 * D + 4 * q); t1 = ldv4(wvec + 2 * D + 16 + 4 * q);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = 32 * half + 16 * u + 4 * q;
        const f32x4_t Az0 = ldv4(wt + (0 * D + a) * kBwT + col), Az1 = ldv4(wt + (0 * D + 16 + a) * kBwT + col);
        const f32x4_t Ar0 = ldv4(wt + (1 * D + a) * kBwT + col), Ar1 = ldv4(wt + (1 * D + 16 + a) * kBwT + col);
        const f32x4_t Bv = half == 0 ? (u == 0 ? h0 : h1) : (u == 0 ? a0 : a1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z0 = mfma_f32(Az0[r], Bv[r], z0);
          z1 = mfma_f32(Az1[r], Bv[r], z1);
          r0 = mfma_f32(Ar0[r], Bv[r], r0);
          r1 = mfma_f32(Ar1[r], Bv[r], r1);
        }
      }
    }
    f32x4_t rh0, rh1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      z0[i] = sigmoid_exact(z0[i]);
      z1[i] = sigmoid_exact(z1[i]);
      r0[i] = sigmoid_exact(r0[i]);
      r1[i] = sigmoid_exact(r1[i]);
      rh0[i] = r0[i] * h0[i];
      rh1[i] = r1[i] * h1[i];
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = 32 * half + 16 * u + 4 * q;
        const f32x4_t Ah0 = ldv4(wt + (2 * D + a) * kBwT + col), Ah1 = ldv4(wt + (2 * D + 16 + a) * kBwT + col);
        const f32x4_t Bv = half == 0 ? (u == 0 ? rh0 : rh1) : (u == 0 ? a0 : a1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t0 = mfma_f32(Ah0[r], Bv[r], t0);
          t1 = mfma_f32(Ah1[r], Bv[r], t1);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t0[i] = tanhf(t0[i]);
      t1[i] = tanhf(t1[i]);
    }
    if (live) {
      stv4(rh_out + row * D + 4 * q, rh0);
      stv4(rh_out + row * D + 16 + 4 * q, rh1);
    }
    }
    f32x4_t n0, n1;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      n0[i] = fmaf(z0[i], t0[i] - h0[i], h0[i]);
      n1[i] = fmaf(z1[i], t1[i] - h1[i], h1[i]);
      sum += n0[i] + n1[i];
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / D);
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      n0[i] -= mean;
      n1[i] -= mean;
      var = fmaf(n0[i], n0[i], var);
      var = fmaf(n1[i], n1[i], var);
    }
    var += __shfl_xor(var, 16);
    var += __shfl_xor(var, 32);
    const float inv = 1.0f / sqrtf(var * (1.0f / D) + eps);
    // ---- LayerNorm backward
    f32x4_t dx0, dx1;
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      n0[i] *= inv;  // x-hat
      n1[i] *= inv;
      dx0[i] = dy0[i] * gm0[i];
      dx1[i] = dy1[i] * gm1[i];
      m1 += dx0[i] + dx1[i];
      m2 = fmaf(dx0[i], n0[i], m2);
      m2 = fmaf(dx1[i], n1[i], m2);
      s_dg[0][i] = fmaf(dy0[i], n0[i], s_dg[0][i]);
      s_dg[1][i] = fmaf(dy1[i], n1[i], s_dg[1][i]);
      s_db[0][i] += dy0[i];
      s_db[1][i] += dy1[i];
    }
    m1 += __shfl_xor(m1, 16);
    m1 += __shfl_xor(m1, 32);
    m2 += __shfl_xor(m2, 16);
    m2 += __shfl_xor(m2, 32);
    m1 *= (1.0f / D);
    m2 *= (1.0f / D);
    f32x4_t dzp0, dzp1, dtp0, dtp1, dh0, dh1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dn0 = inv * (dx0[i] - m1 - n0[i] * m2), dn1 = inv * (dx1[i] - m1 - n1[i] * m2);
      dzp0[i] = dn0 * (t0[i] - h0[i]) * z0[i] * (1.0f - z0[i]);
      dzp1[i] = dn1 * (t1[i] - h1[i]) * z1[i] * (1.0f - z1[i]);
      dtp0[i] = dn0 * z0[i] * (1.0f - t0[i] * t0[i]);
      dtp1[i] = dn1 * z1[i] * (1.0f - t1[i] * t1[i]);
      dh0[i] = dy0[i] + dn0 * (1.0f - z0[i]);
      dh1[i] = dy1[i] + dn1 * (1.0f - z1[i]);
    }
    // ---- dc2 = Wh dtp : rows 0..31 of Wh act on r*h, rows 32..63 on agg
    f32x4_t lo0 = zero4, lo1 = zero4, hi0 = zero4, hi1 = zero4;
    const float* whn = wn + 2 * 2 * D * kBwN;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = 16 * u + 4 * q;
      const f32x4_t A0 = ldv4(whn + (a) * kBwN + col), A1 = ldv4(whn + (16 + a) * kBwN + col);
      const f32x4_t A2 = ldv4(whn + (32 + a) * kBwN + col), A3 = ldv4(whn + (48 + a) * kBwN + col);
      const f32x4_t Bv = u == 0 ? dtp0 : dtp1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        lo0 = mfma_f32(A0[r], Bv[r], lo0);
        lo1 = mfma_f32(A1[r], Bv[r], lo1);
        hi0 = mfma_f32(A2[r], Bv[r], hi0);
        hi1 = mfma_f32(A3[r], Bv[r], hi1);
      }
    }
    f32x4_t drp0, drp1, da0 = hi0, da1 = hi1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      drp0[i] = lo0[i] * h0[i] * r0[i] * (1.0f - r0[i]);
      drp1[i] = lo1[i] * h1[i] * r1[i] * (1.0f - r1[i]);
      dh0[i] = fmaf(lo0[i], r0[i], dh0[i]);
      dh1[i] = fmaf(lo1[i], r1[i], dh1[i]);
      s_bz[0][i] += dzp0[i]; s_bz[1][i] += dzp1[i];
      s_br[0][i] += drp0[i]; s_br[1][i] += drp1[i];
      s_bh[0][i] += dtp0[i]; s_bh[1][i] += dtp1[i];
    }
    // ---- dc = Wz dzp + Wr drp
    lo0 = zero4; lo1 = zero4; hi0 = zero4; hi1 = zero4;
#pragma unroll
    for (int gsel = 0; gsel < 2; ++gsel) {
      const float* wg = wn + gsel * 2 * D * kBwN;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int col = 16 * u + 4 * q;
        const f32x4_t A0 = ldv4(wg + (a) * kBwN + col), A1 = ldv4(wg + (16 + a) * kBwN + col);
        const f32x4_t A2 = ldv4(wg + (32 + a) * kBwN + col), A3 = ldv4(wg + (48 + a) * kBwN + col);
        const f32x4_t Bv = gsel == 0 ? (u == 0 ? dzp0 : dzp1) : (u == 0 ? drp0 : drp1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lo0 = mfma_f32(A0[r], Bv[r], lo0);
          lo1 = mfma_f32(A1[r], Bv[r], lo1);
          hi0 = mfma_f32(A2[r], Bv[r], hi0);
          hi1 = mfma_f32(A3[r], Bv[r], hi1);
        }
      }
    }
    if (live) {
      stv4(dh + row * D + 4 * q, dh0 + lo0);
      stv4(dh + row * D + 16 + 4 * q, dh1 + lo1);
      stv4(dagg + row * D + 4 * q, da0 + hi0);
      stv4(dagg + row * D + 16 + 4 * q, da1 + hi1);
      float* dp = dpre + row * 3 * D;
      stv4(dp + 4 * q, dzp0);
      stv4(dp + 16 + 4 * q, dzp1);
      stv4(dp + D + 4 * q, drp0);
      stv4(dp + D + 16 + 4 * q, drp1);
      stv4(dp + 2 * D + 4 * q, dtp0);
      stv4(dp + 2 * D + 16 + 4 * q, dtp1);
    }
  }
  // ---- column sums: over the 16 rows of a DPP row, then over the 4 waves (fixed order)
  f32x4_t* sums[5] = {s_bz, s_br, s_bh, s_dg, s_db};
#pragma unroll
  for (int w5 = 0; w5 < 5; ++w5)
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = row16_sum_f(sums[w5][blk][i]);
        if (a == 0) red[(wave * 5 + w5) * D + 16 * blk + 4 * q + i] = v;
      }
  __syncthreads();
  float* mine = small + (int64_t)blockIdx.x * 5 * D;
  for (int t = threadIdx.x; t < 5 * D; t += kBlock)
    mine[t] = (red[t] + red[5 * D + t]) + (red[10 * D + t] + red[15 * D + t]);
}

// ---------------------------------------------------------------------------------------
// a7 backward for wide states (D = 64, 128) on the matrix cores: the adjoint of gated_update_wide16_kernel
// (layer_kernels.hip) with its layout - a workgroup of 16 waves owns 64 rows at a time, wave (row tile rt,
// feature group fg) the NT/4 feature tiles 16*(fg*NT/4 + TL) + a of 16 rows; rows on the MFMA M dimension, the
// kernels stream through LDS in double-buffered slices of 16 contraction indices, read as stored for the forward
// recompute and column-wise (W^T) for the products with the pre-activation gradients:
//   P1  z, r   = [h|agg] [Wz|Wr]            P2  t = [r*h|agg] Wh
//   P3  dc2    = dtp Wh^T                    P4  dc = [dzp|drp] [Wz^T ; Wr^T]
// LDS: c = [h|agg] (later [dzp|drp]), r*h (later dtp), two slice buffers, LayerNorm row partials, column sums.
// Outputs and partial sums are those of gated_update_bwd_kernel.
// ---------------------------------------------------------------------------------------
// SAVED: dpre / rh_out arrive holding what the training forward kept (gated_update_wide16_kernel's `save`: z, r, tanh(t)
// in the slots that receive dzp, drp, dtp; r * h) - the recompute passes P1 and P2, half of the kernel's MFMAs, go.
template <int NT, bool SAVED, class... Drop>  // Drop: as gated_update_bwd_kernel
__global__ __launch_bounds__(1024) void gated_update_bwd_wide16_kernel(
    const float* __restrict__ h, const float* __restrict__ agg, const float* __restrict__ Wz,
    const float* __restrict__ bz, const float* __restrict__ Wr, const float* __restrict__ br,
    const float* __restrict__ Wh, const float* __restrict__ bh, const float* __restrict__ gamma, float eps,
    const float* __restrict__ dout, float* __restrict__ dh, float* __restrict__ dagg, float* __restrict__ dpre,
    float* __restrict__ rh_out, float* __restrict__ small, int64_t rows, const int32_t* __restrict__ ridx,
    const int32_t* __restrict__ nrows_dev, float* __restrict__ hc, float* __restrict__ aggc, int tile_rows,
    const float* __restrict__ wt, Drop... drop) {
  // wt = [Wz^T | Wr^T | Wh^T], each D x 2D (transpose3_kernel, once per call): the slices of P3 / P4 are then rows of
  // 2D consecutive floats - fetched and parked like the forward's (coalesced 4-byte loads two slices ahead, one
  // conflict-free 16-byte LDS store, a ring of three buffers) instead of 64-byte pieces and 4-way conflicting stores.
  // tile_rows = 64, or 16 for launches with too few rows to fill the chip with 64-row tiles (the reference trains with
  // 32 pairs per step): then only the four waves of row tile 0 - one per SIMD - run the four GEMM passes.
  // ridx / nrows_dev (optional): the kernel works on the rows ridx[0 .. *nrows_dev) of h / agg / dout / dh / dagg
  // (impnn_gated_update_rows_bwd: the kept rows of an encode() loop); dpre, r*h and the copies hc / aggc of the rows'
  // inputs are written compactly (list position), which is what the weight-gradient GEMMs behind this kernel read.
  const int64_t max_rows = rows;  // what the launch and every buffer are sized for
  if (nrows_dev) {  // a stale or foreign device count never reaches beyond the sizing (indices are never trusted)
    const int64_t n = *nrows_dev;
    rows = n < 0 ? 0 : (n < max_rows ? n : max_rows);
  }
  constexpr int D = 16 * NT, LDC = 2 * D + 4, LDR = D + 4, LDW = 2 * D, NL = NT / 4;
  extern __shared__ __align__(16) float smem[];
  float* cs = smem;                   // 64 x LDC
  float* rhs = cs + 64 * LDC;         // 64 x LDR
  float* ws = rhs + 64 * LDR;         // 3 x 16 x LDW, element (k = 4*qq + r, column c) at ((qq * LDW + c) * 4 + r)
  float* part = ws + 3 * 16 * LDW;    // 4 x (4 x 64): LayerNorm row partials (sum, sq. deviation, m1, m2)
  float* red = ws;                    // 4 row tiles x 5 x D column sums (after the last tile: the slices are dead)
  static_assert(4 * 5 * D <= 3 * 16 * LDW, "column sums alias the slice ring");
  int32_t* grow_s = reinterpret_cast<int32_t*>(part + 4 * 256);  // 64 global rows of the tile
  const int tid = threadIdx.x;
  int a = tid & 15, q = (tid >> 4) & 3, fg = (tid >> 6) & 3, rt = tid >> 8;  // lane = 16 q + a, wave = 4 rt + fg: a row tile's four waves sit on four SIMDs
  const bool act = 16 * (tid >> 8) < tile_rows;  // (wave-uniform) does this wave's row tile hold rows of the tile?
  constexpr int kPre = 16 * 2 * D / 1024;
  float pre[kPre];
  // (`opaque(tid)`: the slice addresses are recomputed where they are used - a few integer ops - instead of being
  //  hoisted out of the GEMM loops by the compiler: ~60 loop-invariant per-thread addresses had been spilled to scratch
  //  in the prologue and reloaded in every iteration)
  auto opaque = [](int v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  auto opaque0 = [](int v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  auto relane = [&]() {  // same values, re-derived: every phase's element addresses start from here
    const int t_ = opaque0(threadIdx.x);
    a = t_ & 15; q = (t_ >> 4) & 3; fg = (t_ >> 6) & 3; rt = t_ >> 8;
  };
  auto park = [&](float* dst, int ncols) {  // slice element t -> (k = t / ncols, column t % ncols)
    const int tid = opaque(threadIdx.x);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int t = tid + 1024 * i;
      if (t < 16 * ncols) {
        const int jj = t / ncols, c = t - jj * ncols;
        dst[(((jj >> 2) * LDW + c) << 2) + (jj & 3)] = pre[i];
      }
    }
  };
  auto park_t = [&](float* dst) {           // transposed slices: element t -> (column t / 16, k = t % 16)
    const int tid = opaque(threadIdx.x);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int t = tid + 1024 * i, c = t >> 4, jj = t & 15;
      dst[(((jj >> 2) * LDW + c) << 2) + (jj & 3)] = pre[i];
    }
  };
  float s_bz[NL] = {}, s_br[NL] = {}, s_bh[NL] = {}, s_dg[NL] = {}, s_db[NL] = {};
  [[maybe_unused]] DropoutKey dk{};
  if constexpr (sizeof...(Drop) > 0) dk = dropout_key(dropout_of(drop...));
  const int64_t ntile = (rows + tile_rows - 1) / tile_rows;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t row0 = tile * tile_rows;
    const int nrt = (int)((rows - row0) < tile_rows ? (rows - row0) : tile_rows);  // rows of this tile
    // per-tile base pointers (scalar) + 32-bit offsets: keeps the per-element addresses out of the register file
    float* rh_t = rh_out + row0 * D;
    float* dpre_t = dpre + row0 * 3 * D;
    __syncthreads();
    if (tid < 64) {
      int64_t gr = tid < nrt ? (ridx ? (int64_t)ridx[row0 + tid] : row0 + tid) : 0;
      grow_s[tid] = (int32_t)(gr < 0 ? 0 : (gr < max_rows ? gr : max_rows - 1));
    }
    __syncthreads();
    // dropout: the forward's keep bits of this lane's 4 x NL elements (bit 4 TL + g), drawn while few registers are live
    [[maybe_unused]] uint32_t keep = 0;
    if constexpr (sizeof...(Drop) > 0) {
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        uint32_t mw[4];
        dropout_quad_words(dk, grow_s[16 * rt + 4 * q + (a & 3)], (16 * (fg * NL + TL) + a) >> 2, a & 3, mw);
#pragma unroll
        for (int g = 0; g < 4; ++g) keep |= (uint32_t)((mw[g] >> 8) >= dk.thr) << (4 * TL + g);
      }
    }
    for (int t = tid; t < 64 * D; t += 1024) {
      const int r = t / D, c = t - r * D;
      const bool in = r < nrt;
      const int64_t src = (int64_t)grow_s[r] * D + c;
      const float hv = in ? h[src] : 0.f, av = in ? agg[src] : 0.f;
      cs[r * LDC + c] = hv;
      cs[r * LDC + D + c] = av;
#ifndef IMPNN_DIAG_GUB_NOCOPY
      if (hc && in) {
        hc[row0 * D + t] = hv;
        aggc[row0 * D + t] = av;
      }
#endif
    }
    const float* crow = cs + (16 * rt + a) * LDC + 4 * q;
    const float* rrow = rhs + (16 * rt + a) * LDR + 4 * q;
    f32x4_t tt[NL];
    if constexpr (SAVED) {
      __syncthreads();  // the tile of [h | agg] is in LDS
    } else {
    // ---- P1: z, r
    f32x4_t z[NL], rr[NL];
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      const int f = 16 * (fg * NL + TL) + a;
      z[TL] = f32x4_t{bz[f], bz[f], bz[f], bz[f]};
      rr[TL] = f32x4_t{br[f], br[f], br[f], br[f]};
    }
    auto fetch1 = [&](int u) {
      const int tid = opaque(threadIdx.x);
#pragma unroll
      for (int i = 0; i < kPre; ++i) {
        const int t = tid + 1024 * i, jj = t / (2 * D), c = t - jj * 2 * D;
        pre[i] = c < D ? Wz[(int64_t)(16 * u + jj) * D + c] : Wr[(int64_t)(16 * u + jj) * D + c - D];
      }
    };
    fetch1(0);
    park(ws, 2 * D);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < 2 * NT; ++u) {
      float* cur = ws + (u & 1) * 16 * LDW;
      float* nxt = ws + ((u + 1) & 1) * 16 * LDW;
      if (u + 1 < 2 * NT) fetch1(u + 1);
      if (act) {
      const f32x4_t av = ldv4(crow + 16 * u);
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const int col = 16 * (fg * NL + TL) + a;
        const f32x4_t b0 = ldv4(cur + ((q * LDW + col) << 2)), b1 = ldv4(cur + ((q * LDW + D + col) << 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z[TL] = mfma_f32(av[r], b0[r], z[TL]);
          rr[TL] = mfma_f32(av[r], b1[r], rr[TL]);
        }
      }
      }
      if (u + 1 < 2 * NT) park(nxt, 2 * D);
      __syncthreads();
    }
    relane();
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g, f = 16 * (fg * NL + TL) + a;
        z[TL][g] = sigmoid_exact(z[TL][g]);
        rr[TL][g] = sigmoid_exact(rr[TL][g]);
        const float v = rr[TL][g] * cs[rl * LDC + f];
        rhs[rl * LDR + f] = v;
        if (rl < nrt) rh_t[rl * D + f] = v;
        // Register relief (the kernel ran 156 VGPRs over its 128 with everything held): r, z and tanh(t) are parked
        // in the tile's own dpre rows - slots that receive drp / dzp / dtp later anyway - and read back by the same
        // thread where they are needed again (L2-resident, same address: program order).
        if (rl < nrt) {
          dpre_t[rl * 3 * D + D + f] = rr[TL][g];
          dpre_t[rl * 3 * D + f] = z[TL][g];
        }
      }
    // ---- P2: t
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      const float b2 = bh[16 * (fg * NL + TL) + a];
      tt[TL] = f32x4_t{b2, b2, b2, b2};
    }
    auto fetch2 = [&](int u) {
      const int tid = opaque(threadIdx.x);
#pragma unroll
      for (int i = 0; i < kPre; ++i) {
        const int t = tid + 1024 * i;
        if (t < 16 * D) pre[i] = Wh[(int64_t)(16 * u + t / D) * D + t % D];
      }
    };
    fetch2(0);
    park(ws, D);
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < 2 * NT; ++u) {
      float* cur = ws + (u & 1) * 16 * LDW;
      float* nxt = ws + ((u + 1) & 1) * 16 * LDW;
      if (u + 1 < 2 * NT) fetch2(u + 1);
      if (act) {
      const f32x4_t av = u < NT ? ldv4(rrow + 16 * u) : ldv4(crow + 16 * u);
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const f32x4_t bv = ldv4(cur + ((q * LDW + 16 * (fg * NL + TL) + a) << 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) tt[TL] = mfma_f32(av[r], bv[r], tt[TL]);
      }
      }
      if (u + 1 < 2 * NT) park(nxt, D);
      __syncthreads();
    }
    }
    // ---- blend, LayerNorm forward statistics
    relane();
    f32x4_t xh[NL];
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g, f = 16 * (fg * NL + TL) + a;
        const float hv = cs[rl * LDC + f];
        float tv;
        if constexpr (SAVED) tv = rl < nrt ? dpre_t[rl * 3 * D + 2 * D + f] : 0.f;
        else tv = tanhf(tt[TL][g]);
        const float zz = rl < nrt ? dpre_t[rl * 3 * D + f] : 0.f;
        xh[TL][g] = (1.0f - zz) * hv + zz * tv;
        sum[g] += xh[TL][g];
        if (!SAVED && rl < nrt) dpre_t[rl * 3 * D + 2 * D + f] = tv;
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float v = row16_sum_f(sum[g]);
      if (a == 0) part[fg * 64 + 16 * rt + 4 * q + g] = v;
    }
    __syncthreads();
    float mean[4], inv[4], var[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl = 16 * rt + 4 * q + g;
      mean[g] = ((part[rl] + part[64 + rl]) + (part[128 + rl] + part[192 + rl])) * (1.0f / D);
    }
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        xh[TL][g] -= mean[g];
        var[g] = fmaf(xh[TL][g], xh[TL][g], var[g]);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float v = row16_sum_f(var[g]);
      if (a == 0) part[256 + fg * 64 + 16 * rt + 4 * q + g] = v;
    }
    __syncthreads();
    float m1[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl = 256 + 16 * rt + 4 * q + g;
      inv[g] = 1.0f / sqrtf(((part[rl] + part[64 + rl]) + (part[128 + rl] + part[192 + rl])) * (1.0f / D) + eps);
    }
    // ---- LayerNorm backward
    relane();
    f32x4_t dxh[NL], dy[NL];
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      const float gm = gamma[16 * (fg * NL + TL) + a];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g;
        dy[TL][g] = rl < nrt ? dout[(int64_t)grow_s[rl] * D + 16 * (fg * NL + TL) + a] : 0.f;
        if constexpr (sizeof...(Drop) > 0) dy[TL][g] = (keep >> (4 * TL + g)) & 1u ? dy[TL][g] * dk.scale : 0.0f;
        xh[TL][g] *= inv[g];
        dxh[TL][g] = dy[TL][g] * gm;
        m1[g] += dxh[TL][g];
        m2[g] = fmaf(dxh[TL][g], xh[TL][g], m2[g]);
        s_dg[TL] = fmaf(dy[TL][g], xh[TL][g], s_dg[TL]);
        s_db[TL] += dy[TL][g];
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float v1 = row16_sum_f(m1[g]), v2 = row16_sum_f(m2[g]);
      if (a == 0) {
        part[512 + fg * 64 + 16 * rt + 4 * q + g] = v1;
        part[768 + fg * 64 + 16 * rt + 4 * q + g] = v2;
      }
    }
    __syncthreads();  // (also: every wave is done reading r*h from `rhs`)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int rl = 16 * rt + 4 * q + g;
      m1[g] = ((part[512 + rl] + part[576 + rl]) + (part[640 + rl] + part[704 + rl])) * (1.0f / D);
      m2[g] = ((part[768 + rl] + part[832 + rl]) + (part[896 + rl] + part[960 + rl])) * (1.0f / D);
    }
    relane();
    f32x4_t dhA[NL];
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g, f = 16 * (fg * NL + TL) + a;
        const float hv = cs[rl * LDC + f];
        const float dn = inv[g] * (dxh[TL][g] - m1[g] - xh[TL][g] * m2[g]);
        const float zz = rl < nrt ? dpre_t[rl * 3 * D + f] : 0.f, tv = rl < nrt ? dpre_t[rl * 3 * D + 2 * D + f] : 0.f;
        const float dzp = dn * (tv - hv) * zz * (1.0f - zz);
        const float dtp = dn * zz * (1.0f - tv * tv);
        dhA[TL][g] = dy[TL][g] + dn * (1.0f - zz);
        s_bz[TL] += dzp;
        s_bh[TL] += dtp;
        rhs[rl * LDR + f] = dtp;  // A operand of P3
        if (rl < nrt) {
          dpre_t[rl * 3 * D + f] = dzp;
          dpre_t[rl * 3 * D + 2 * D + f] = dtp;
        }
      }
    // ---- P3: dc2 = dtp Wh^T  (lo: through r*h, hi: to agg)
    f32x4_t lo[NL], hi[NL];
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) lo[TL] = hi[TL] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // slices of a transposed kernel (rows k0 .. k0 + 15 of a D x 2D block of wt): thread (qq, c) moves rows 4qq .. 4qq + 3
    // of column c
    constexpr int kIT = 4 * 2 * D;
    static_assert(kIT <= 1024, "one item per thread");
    auto fetchT = [&](const float* base, int k0, f32x4_t& pre4) {
      const int t_ = opaque(threadIdx.x);
      if (t_ < kIT) {
        const int qq = t_ / (2 * D), c = t_ - qq * (2 * D);
        const float* src = base + (int64_t)(k0 + 4 * qq) * (2 * D) + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) pre4[r] = src[r * 2 * D];
      }
    };
    auto parkT = [&](float* dst, const f32x4_t& pre4) {
      const int t_ = opaque(threadIdx.x);
      if (t_ < kIT) {
        const int qq = t_ / (2 * D), c = t_ - qq * (2 * D);
        *reinterpret_cast<f32x4_t*>(dst + ((qq * LDW + c) << 2)) = pre4;
      }
    };
    struct OpsT {
      f32x4_t av, b0[NL], b1[NL];
    };
    auto readT = [&](const float* arow, int u, OpsT& o) {
      const float* cur = ws + (u % 3) * 16 * LDW;
      o.av = ldv4(arow + 16 * u);
#pragma unroll
      for (int TL = 0; TL < NL; ++TL) {
        const int col = 16 * (fg * NL + TL) + a;
        o.b0[TL] = ldv4(cur + ((q * LDW + col) << 2));
        o.b1[TL] = ldv4(cur + ((q * LDW + D + col) << 2));
      }
    };
    auto mmaT = [&](const OpsT& o) {
      if (!act) return;
#pragma unroll
      for (int TL = 0; TL < NL; ++TL)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lo[TL] = mfma_f32(o.av[r], o.b0[TL][r], lo[TL]);
          hi[TL] = mfma_f32(o.av[r], o.b1[TL][r], hi[TL]);
        }
    };
    // [lo | hi] += A (rows of `arow`, 16 nsl contraction indices) x the nsl slices that start at `base`
    auto passT = [&](const float* base, int nsl, const float* arow) {
#ifdef IMPNN_DIAG_GUB_NOGEMM  // (knock-out timing builds: tools/gu_pair_bench.py with IMPNN_LIB)
      return;
#endif
      f32x4_t preA, preB;
      fetchT(base, 0, preA);
      fetchT(base, 16, preB);
      parkT(ws, preA);
      __syncthreads();
#pragma unroll 1
      for (int u = 0; u < nsl; u += 2) {
        OpsT o;
        if (u + 2 < nsl) fetchT(base, 16 * (u + 2), preA);
        readT(arow, u, o);
        __builtin_amdgcn_sched_barrier(0);
        parkT(ws + ((u + 1) % 3) * 16 * LDW, preB);
        __builtin_amdgcn_sched_barrier(0);
        mmaT(o);
        __syncthreads();
        if (u + 3 < nsl) fetchT(base, 16 * (u + 3), preB);
        readT(arow, u + 1, o);
        __builtin_amdgcn_sched_barrier(0);
        if (u + 2 < nsl) parkT(ws + ((u + 2) % 3) * 16 * LDW, preA);
        __builtin_amdgcn_sched_barrier(0);
        mmaT(o);
        __syncthreads();
      }
    };
    passT(wt + (int64_t)2 * 2 * D * D, NT, rrow);
    relane();
    // lo / hi go on as P4's accumulators: they start from the direct terms (dh: dy + dn (1 - z) + r dc2_lo, dagg: dc2_hi).
    // c = [h | agg] becomes [dzp | drp] element by element - a thread reads and replaces its own h, nobody reads agg
    // after P2 - so only the barrier in front of P4's first operand read is needed.
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g, f = 16 * (fg * NL + TL) + a;
        const float hv = cs[rl * LDC + f], rv = rl < nrt ? dpre_t[rl * 3 * D + D + f] : 0.f;
        const float dzp = rl < nrt ? dpre_t[rl * 3 * D + f] : 0.f;  // parked above
        const float drp = lo[TL][g] * hv * rv * (1.0f - rv);
        s_br[TL] += drp;
        if (rl < nrt) dpre_t[rl * 3 * D + D + f] = drp;
        cs[rl * LDC + f] = dzp;
        cs[rl * LDC + D + f] = drp;
        lo[TL][g] = fmaf(lo[TL][g], rv, dhA[TL][g]);
      }
    // ---- P4: dc = [dzp|drp] [Wz^T ; Wr^T]
    passT(wt, 2 * NT, crow);  // [Wz^T ; Wr^T] are consecutive rows of wt
    relane();
#pragma unroll
    for (int TL = 0; TL < NL; ++TL)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 16 * rt + 4 * q + g, f = 16 * (fg * NL + TL) + a;
        if (rl < nrt) {
          const int64_t dst = (int64_t)grow_s[rl] * D + f;
          dh[dst] = lo[TL][g];
          dagg[dst] = hi[TL][g];
        }
      }
  }
  // ---- column sums: the 4 row quarters of a wave, then the 4 row tiles (fixed order)
  float* sums[5] = {s_bz, s_br, s_bh, s_dg, s_db};
#pragma unroll
  for (int w5 = 0; w5 < 5; ++w5)
#pragma unroll
    for (int TL = 0; TL < NL; ++TL) {
      float v = sums[w5][TL];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (q == 0) red[(rt * 5 + w5) * D + 16 * (fg * NL + TL) + a] = v;
    }
  __syncthreads();
  float* mine = small + (int64_t)blockIdx.x * 5 * D;
  for (int t = tid; t < 5 * D; t += 1024)
    mine[t] = (red[t] + red[5 * D + t]) + (red[10 * D + t] + red[15 * D + t]);
}

// WT = [Wz^T | Wr^T | Wh^T] (each D x 2D) for the large-D variant above (32x32 LDS tiles)
__global__ void transpose3_kernel(const float* __restrict__ Wz, const float* __restrict__ Wr,
                                  const float* __restrict__ Wh, float* __restrict__ WT, int D) {
  __shared__ float tile[32][33];
  const float* W = blockIdx.z == 0 ? Wz : (blockIdx.z == 1 ? Wr : Wh);
  float* T = WT + (int64_t)blockIdx.z * 2 * D * D;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;  // W is (2D x D): rows r, cols c
  for (int y = threadIdx.y; y < 32; y += blockDim.y) {
    const int r = r0 + y, c = c0 + threadIdx.x;
    tile[y][threadIdx.x] = (r < 2 * D && c < D) ? W[(int64_t)r * D + c] : 0.f;
  }
  __syncthreads();
  for (int y = threadIdx.y; y < 32; y += blockDim.y) {
    const int c = c0 + y, r = r0 + threadIdx.x;       // T is (D x 2D): T[c][r]
    if (c < D && r < 2 * D) T[(int64_t)c * 2 * D + r] = tile[threadIdx.x][y];
  }
}

// C[M x N] (per chunk) = sum over the chunk's rows r of A(r,m) * B(r,n), every operand addressed with a row and
// a column stride; the M axis may be the concatenation [A1 | A2] of two operands (split at Mh).
// blockIdx = (chunk, tile, problem); 64 x 32 output tile, thread owns 4 x 2, 32 rows staged in LDS per iteration.
// Output of chunk c of problem p: out + (p * nchunk + c) * M * N, row-major.
struct GemmProblems {
  const float* A1[3];
  const float* A2[3];
  const float* B[3];
};
constexpr int kGM = 64, kGN = 32, kGR = 32;  // output tile, rows staged per iteration

__global__ __launch_bounds__(kBlock) void strided_gemm_splitk_kernel(GemmProblems ga, float* __restrict__ out,
                                                                     int64_t rows, int M, int Mh, int N,
                                                                     int64_t a_rs, int64_t a_cs, int64_t b_rs,
                                                                     int64_t b_cs, int nchunk, int tilesN,
                                                                     const int32_t* __restrict__ rows_dev) {
  if (rows_dev) {  // (the contraction length lives on the device: kept rows of a batch; never beyond the sizing)
    const int64_t n = *rows_dev;
    rows = n < 0 ? 0 : (n < rows ? n : rows);
  }
  // LDS tiles of kGR contraction rows; row strides chosen so that the four k-rows of one MFMA step fall into
  // disjoint bank groups (80 = 64 + 16, 48 = 32 + 16 floats)
  constexpr int kLA = kGM + 16, kLB = kGN + 16;
  __shared__ __align__(16) float As[kGR * kLA];
  __shared__ __align__(16) float Bs[kGR * kLB];
  const int chunk = blockIdx.x, tile = blockIdx.y, prob = blockIdx.z;
  const int tm0 = (tile / tilesN) * kGM, tn0 = (tile % tilesN) * kGN;
  const float* A1 = ga.A1[prob];
  const float* A2 = ga.A2[prob];
  const float* B = ga.B[prob];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  const int64_t per = (rows + nchunk - 1) / nchunk;
  const int64_t r_lo = (int64_t)chunk * per, r_hi = r_lo + per < rows ? r_lo + per : rows;
  // exact-f32 MFMA: wave w owns output rows m = 16w .. 16w+15 of the 64 x 32 tile (two 16 x 16 tiles);
  // contraction rows on K: lane (a, q) feeds A[row 4s+q][16w + a] and B[row 4s+q][16t + a] straight from the tiles
  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  // Fast path (the GatedUpdate weight gradients: both operands row-major, whole tiles): 16-byte loads, the next
  // kGR rows in flight in registers under the MFMAs of the current ones.
  const bool fast = a_cs == 1 && b_cs == 1 && tm0 + kGM <= M && tn0 + kGN <= N && (Mh & 3) == 0 && (a_rs & 3) == 0 &&
                    (b_rs & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(A1) | reinterpret_cast<uintptr_t>(A2) | reinterpret_cast<uintptr_t>(B)) & 15u) == 0;
  if (fast) {
    constexpr int kA4 = kGR * kGM / 4 / kBlock, kB4 = kGR * kGN / 4 / kBlock;  // float4 per thread: 2 and 1
    static_assert(kA4 * kBlock * 4 == kGR * kGM && kB4 * kBlock * 4 == kGR * kGN, "tile / block mismatch");
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t ra[kA4], rb[kB4];
    const float* ap[kA4];
    const float* bp[kB4];
    int ar[kA4], br_[kB4], ao[kA4], bo[kB4];
#pragma unroll
    for (int i = 0; i < kA4; ++i) {
      const int t = tid + kBlock * i, r = t / (kGM / 4), m = tm0 + 4 * (t % (kGM / 4));
      ar[i] = r;
      ao[i] = r * kLA + 4 * (t % (kGM / 4));
      ap[i] = (m < Mh ? A1 + m : A2 + (m - Mh)) + (int64_t)r * a_rs;
    }
#pragma unroll
    for (int i = 0; i < kB4; ++i) {
      const int t = tid + kBlock * i, r = t / (kGN / 4), n = tn0 + 4 * (t % (kGN / 4));
      br_[i] = r;
      bo[i] = r * kLB + 4 * (t % (kGN / 4));
      bp[i] = B + n + (int64_t)r * b_rs;
    }
    auto fetch = [&](int64_t r0) {
      const int nr = (int)((r_hi - r0) < kGR ? (r_hi - r0) : kGR);
#pragma unroll
      for (int i = 0; i < kA4; ++i)
        ra[i] = ar[i] < nr ? *reinterpret_cast<const f32x4_t*>(ap[i] + r0 * a_rs) : zero4;
#pragma unroll
      for (int i = 0; i < kB4; ++i)
        rb[i] = br_[i] < nr ? *reinterpret_cast<const f32x4_t*>(bp[i] + r0 * b_rs) : zero4;
    };
    if (r_lo < r_hi) fetch(r_lo);
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += kGR) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kA4; ++i) *reinterpret_cast<f32x4_t*>(As + ao[i]) = ra[i];
#pragma unroll
      for (int i = 0; i < kB4; ++i) *reinterpret_cast<f32x4_t*>(Bs + bo[i]) = rb[i];
      __syncthreads();
      if (r0 + kGR < r_hi) fetch(r0 + kGR);
#pragma unroll
      for (int st = 0; st < kGR / 4; ++st) {
        const float av = As[(4 * st + q) * kLA + 16 * wave + a];
        const float b0 = Bs[(4 * st + q) * kLB + a], b1 = Bs[(4 * st + q) * kLB + 16 + a];
        acc0 = mfma_f32(av, b0, acc0);
        acc1 = mfma_f32(av, b1, acc1);
      }
    }
  } else
  for (int64_t r0 = r_lo; r0 < r_hi; r0 += kGR) {
    const int nr = (int)((r_hi - r0) < kGR ? (r_hi - r0) : kGR);
    __syncthreads();
    if (a_cs == 1) {  // columns contiguous: lanes walk m
      for (int t = tid; t < kGR * kGM; t += kBlock) {
        const int r = t / kGM, mm = t % kGM, m = tm0 + mm;
        float v = 0.f;
        if (r < nr && m < M) v = m < Mh ? A1[(r0 + r) * a_rs + m] : A2[(r0 + r) * a_rs + (m - Mh)];
        As[r * kLA + mm] = v;
      }
    } else {          // rows contiguous (a transposed operand): lanes walk r
      for (int t = tid; t < kGR * kGM; t += kBlock) {
        const int mm = t / kGR, r = t % kGR, m = tm0 + mm;
        float v = 0.f;
        if (r < nr && m < M) v = m < Mh ? A1[(r0 + r) * a_rs + m * a_cs] : A2[(r0 + r) * a_rs + (m - Mh) * a_cs];
        As[r * kLA + mm] = v;
      }
    }
    if (b_cs == 1) {
      for (int t = tid; t < kGR * kGN; t += kBlock) {
        const int r = t / kGN, nn = t % kGN, n = tn0 + nn;
        Bs[r * kLB + nn] = (r < nr && n < N) ? B[(r0 + r) * b_rs + n] : 0.f;
      }
    } else {
      for (int t = tid; t < kGR * kGN; t += kBlock) {
        const int nn = t / kGR, r = t % kGR, n = tn0 + nn;
        Bs[r * kLB + nn] = (r < nr && n < N) ? B[(r0 + r) * b_rs + n * b_cs] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int st = 0; st < kGR / 4; ++st) {
      const float av = As[(4 * st + q) * kLA + 16 * wave + a];
      const float b0 = Bs[(4 * st + q) * kLB + a], b1 = Bs[(4 * st + q) * kLB + 16 + a];
      acc0 = mfma_f32(av, b0, acc0);
      acc1 = mfma_f32(av, b1, acc1);
    }
  }
  float* o = out + ((int64_t)prob * nchunk + chunk) * M * N;
#pragma unroll
  for (int g = 0; g < 4; ++g) {  // accumulator: row 16w + 4q + g, column 16t + a
    const int m = tm0 + 16 * wave + 4 * q + g;
    if (m < M) {
      if (tn0 + a < N) o[(int64_t)m * N + tn0 + a] = acc0[g];
      if (tn0 + 16 + a < N) o[(int64_t)m * N + tn0 + 16 + a] = acc1[g];
    }
  }
}

// The same product for wide states (M = 2D >= 128, N = D >= 64, both operands row-major, whole tiles): a 128 x 64
// output tile per workgroup, a 32 x 64 block (2 x 4 accumulator tiles) per wave - 6 LDS reads feed 8 MFMAs per k step
// instead of 3 feeding 2, and a 32-row stage holds 64 MFMAs per wave between its two barriers instead of 16 (the
// 64 x 32 tiles above ran the D = 128 weight gradients at 27 % of the f32 MFMA peak: 433 us per call at batch 4096).
constexpr int kBM = 128, kBN = 64;
__global__ __launch_bounds__(kBlock) void strided_gemm_splitk_big_kernel(GemmProblems ga, float* __restrict__ out,
                                                                         int64_t rows, int M, int Mh, int N,
                                                                         int64_t a_rs, int64_t b_rs, int nchunk,
                                                                         int tilesN, const int32_t* __restrict__ rows_dev) {
  if (rows_dev) {
    const int64_t n = *rows_dev;
    rows = n < 0 ? 0 : (n < rows ? n : rows);
  }
  constexpr int kLA = kBM + 16, kLB = kBN + 16;  // row strides: the four k rows of an MFMA step on disjoint bank groups
  __shared__ __align__(16) float As[kGR * kLA];
  __shared__ __align__(16) float Bs[kGR * kLB];
  const int chunk = blockIdx.x, tile = blockIdx.y, prob = blockIdx.z;
  const int tm0 = (tile / tilesN) * kBM, tn0 = (tile % tilesN) * kBN;
  const float* A1 = ga.A1[prob];
  const float* A2 = ga.A2[prob];
  const float* B = ga.B[prob];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  const int64_t per = (rows + nchunk - 1) / nchunk;
  const int64_t r_lo = (int64_t)chunk * per, r_hi = r_lo + per < rows ? r_lo + per : rows;
  constexpr int kA4 = kGR * kBM / 4 / kBlock, kB4 = kGR * kBN / 4 / kBlock;  // float4 per thread: 4 and 2
  static_assert(kA4 * kBlock * 4 == kGR * kBM && kB4 * kBlock * 4 == kGR * kBN, "tile / block mismatch");
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4_t acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = zero4;
  f32x4_t ra[kA4], rb[kB4];
  auto fetch = [&](int64_t r0) {
    const int nr = (int)((r_hi - r0) < kGR ? (r_hi - r0) : kGR);
#pragma unroll
    for (int i = 0; i < kA4; ++i) {
      const int t = tid + kBlock * i, r = t / (kBM / 4), m = tm0 + 4 * (t % (kBM / 4));
      const float* ap = (m < Mh ? A1 + m : A2 + (m - Mh)) + (r0 + r) * a_rs;
      ra[i] = r < nr ? ldv4(ap) : zero4;
    }
#pragma unroll
    for (int i = 0; i < kB4; ++i) {
      const int t = tid + kBlock * i, r = t / (kBN / 4), n = tn0 + 4 * (t % (kBN / 4));
      rb[i] = r < nr ? ldv4(B + n + (r0 + r) * b_rs) : zero4;
    }
  };
  if (r_lo < r_hi) fetch(r_lo);
  for (int64_t r0 = r_lo; r0 < r_hi; r0 += kGR) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kA4; ++i) {
      const int t = tid + kBlock * i;
      stv4(As + (t / (kBM / 4)) * kLA + 4 * (t % (kBM / 4)), ra[i]);
    }
#pragma unroll
    for (int i = 0; i < kB4; ++i) {
      const int t = tid + kBlock * i;
      stv4(Bs + (t / (kBN / 4)) * kLB + 4 * (t % (kBN / 4)), rb[i]);
    }
    __syncthreads();
    if (r0 + kGR < r_hi) fetch(r0 + kGR);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < kGR / 4; ++st) {
      float av[2], bv[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = As[(4 * st + q) * kLA + 32 * wave + 16 * i + a];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = Bs[(4 * st + q) * kLB + 16 * j + a];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma_f32(av[i], bv[j], acc[i][j]);
    }
  }
  float* o = out + ((int64_t)prob * nchunk + chunk) * M * N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // accumulator (i, j): row 32w + 16i + 4q + g, column 16j + a
      const int m = tm0 + 32 * wave + 16 * i + 4 * q + g;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[(int64_t)m * N + tn0 + 16 * j + a] = acc[i][j][g];
    }
}

// dparams = fixed-order sums of the partials (canonical layout, see above).  One wave per output: lane l adds
// partials l, l+64, ... in order, then a fixed butterfly - the same association on every run.
__global__ void gated_update_reduce_kernel(const float* __restrict__ small, const float* __restrict__ gpart,
                                           float* __restrict__ dparams, int nblk, int nchunk, int D, int accumulate,
                                           int wblocks) {
  const int DD2 = 2 * D * D;
  if ((int)blockIdx.x < wblocks) {
    // the three kernel gradients.  Few chunk partials (wide states: <= 64): one THREAD per element, the partials added
    // in chunk order, consecutive threads on consecutive addresses (one wave per element read its 20 partials 128 KB
    // apart: 27 us per call for 8 MB).  Many partials (atom_dim 32 at large batches: 342): one wave per element.
    if (nchunk <= 64) {
      const int t = blockIdx.x * blockDim.x + threadIdx.x;
      if (t >= 3 * DD2) return;
      const int gate = t / DD2, off = t - gate * DD2;
      const float* src = gpart + (int64_t)gate * nchunk * DD2 + off;
      float acc = 0.f;
      int c = 0;
      for (; c + 8 <= nchunk; c += 8) {  // 8 partials in flight, added in chunk order
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = src[(int64_t)(c + u) * DD2];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += x[u];
      }
      for (; c < nchunk; ++c) acc += src[(int64_t)c * DD2];
      const int q = gate * (DD2 + D) + off;
      dparams[q] = accumulate ? dparams[q] + acc : acc;
      return;
    }
    const int t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (t >= 3 * DD2) return;
    const int gate = t / DD2, off = t - gate * DD2;
    const float* src = gpart + (int64_t)gate * nchunk * DD2 + off;
    float acc = 0.f;
    for (int c = lane; c < nchunk; c += 64) acc += src[(int64_t)c * DD2];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    const int q = gate * (DD2 + D) + off;
    if (lane == 0) dparams[q] = accumulate ? dparams[q] + acc : acc;
    return;
  }
  // the five vectors (bz, br, bh, gamma, beta): one wave per element over the nblk per-workgroup column sums
  const int e = (((int)blockIdx.x - wblocks) * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (e >= 5 * D) return;
  const int q = e < 3 * D ? (e / D) * (DD2 + D) + DD2 + (e % D) : 3 * (DD2 + D) + (e - 3 * D);
  const float* src = small + e;
  float acc = 0.f;
  int c = lane;
  for (; c + 7 * 64 < nblk; c += 8 * 64) {  // eight slices in flight (a lane's loads are 5 D floats apart), added in order
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = src[(int64_t)(c + 64 * u) * 5 * D];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += x[u];
  }
  for (; c < nblk; c += 64) acc += src[(int64_t)c * 5 * D];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) dparams[q] = accumulate ? dparams[q] + acc : acc;
}

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

// out[M x N] = sum_r A(r,m) B(r,n) in one pass (no split: deterministic, no workspace)
int launch_strided_gemm(const float* A, const float* B, float* out, int64_t rows, int M, int N, int64_t a_rs,
                        int64_t a_cs, int64_t b_rs, int64_t b_cs, hipStream_t s) {
  GemmProblems ga{};
  ga.A1[0] = A; ga.A2[0] = A; ga.B[0] = B;
  const int tiles_n = (N + kGN - 1) / kGN, tiles_m = (M + kGM - 1) / kGM;
  strided_gemm_splitk_kernel<<<dim3(1, tiles_m * tiles_n, 1), kBlock, 0, s>>>(ga, out, rows, M, M, N, a_rs, a_cs, b_rs,
                                                                              b_cs, 1, tiles_n, nullptr);
  return check_launch("strided_gemm");
}

int launch_bond_type_matrices_bwd(const float* tb, const float* W, const float* dA, float* dW, float* dtb, int Vb,
                                  int K, int D, int accumulate, hipStream_t s) {
  const int DD = D * D;
  if (K >= 64) {
    if (accumulate) return fail(IMPNN_E_UNSUPPORTED, "bond_type_matrices_bwd: accumulate needs K < 64");  // GEMM-shaped: dW (K x DD) = Tb^T dA over Vb rows; dTb (Vb x K) = dA W^T over DD rows
    if (int rc = launch_strided_gemm(tb, dA, dW, Vb, K, DD, K, 1, DD, 1, s)) return rc;
    return launch_strided_gemm(dA, W, dtb, DD, Vb, K, 1, DD, 1, DD, s);
  }
  bond_type_matrices_bwd_w_kernel<<<dim3((DD + kBlock - 1) / kBlock, K), kBlock, 0, s>>>(tb, dA, dW, Vb, K, DD, accumulate);
  if (int rc = check_launch("bond_type_matrices_bwd_w")) return rc;
  const int64_t waves = (int64_t)Vb * K;
  bond_type_matrices_bwd_t_kernel<<<(int)((waves * 64 + kBlock - 1) / kBlock), kBlock, 0, s>>>(W, dA, dtb, Vb, K, DD,
                                                                                               accumulate);
  return check_launch("bond_type_matrices_bwd_t");
}

static int gu_main_blocks(int64_t rows, int D) {
  // tiles of the main kernel: kBlock / D rows (generic kernels), 16 or 64 rows (the wide matrix-core kernel)
  const int R = (D == 64 || D == 128) ? gu_wide_tile_rows(rows) : kBlock / D;
  const int64_t ntile = (rows + R - 1) / R;
  return (int)(ntile < 1024 ? (ntile < 1 ? 1 : ntile) : 1024);
}
// 128 x 64 output tiles: atom_dim 64 / 128 from 8 K rows (below that the 64 x 32 tiles give 4x the workgroups: 1.445
// vs 1.478 ms per step at batch 32)
static bool gu_big_tiles(int D, int64_t rows) { return D % kBN == 0 && (2 * D) % kBM == 0 && rows >= 8192; }
static int gu_tiles(int D, int64_t rows, int* tiles_n) {
  const int gn = gu_big_tiles(D, rows) ? kBN : kGN, gm = gu_big_tiles(D, rows) ? kBM : kGM;
  const int tn = (D + gn - 1) / gn, tm = (2 * D + gm - 1) / gm;
  if (tiles_n) *tiles_n = tn;
  return tm * tn;
}
static int gu_chunks(int64_t rows, int D) {
  const int tiles = gu_tiles(D, rows, nullptr);
  // ~1024 workgroups of the 64 x 32 tiles, ~768 (three resident per CU) of the 128 x 64 ones
  int64_t want = gu_big_tiles(D, rows) ? (768 + 3 * tiles - 1) / (3 * tiles) : (1024 + 3 * tiles - 1) / (3 * tiles);
  const int64_t cap = (rows + 255) / 256;  // at least 256 contraction rows per chunk: fewer partials to write and add
  if (want > cap) want = cap;
  return (int)(want < 1 ? 1 : want);
}

int gated_update_bwd_blocks(int64_t rows, int D) { return gu_main_blocks(rows, D); }

int64_t gated_update_param_floats(int D) { return 3 * ((int64_t)2 * D * D + D) + 2 * D; }

// workspace (floats): dpre rows*3D | r*h rows*D | small nblk*5D | GEMM partials 3*nchunk*2D*D | W^T 3*2D*D
// (row-list form: + compact copies of the rows' h and agg, rows*2D)
int64_t gated_update_bwd_workspace(int64_t rows, int D, bool row_list) {
  return rows * 4 * D + (int64_t)gu_main_blocks(rows, D) * 5 * D + (int64_t)3 * gu_chunks(rows, D) * 2 * D * D +
         (int64_t)3 * 2 * D * D + (row_list ? rows * 2 * D : 0);
}

// (api.hip has checked the call: atom_dim divides 256, and a row list or a `saved` buffer comes with an atom_dim and
// alignment it covers)
template <class... Drop>
static int launch_gated_update_bwd_impl(const GatedUpdateCall& c, Drop... drop) {
  const float *h = c.h, *agg = c.agg, *Wz = c.Wz, *bz = c.bz, *Wr = c.Wr, *br = c.br, *Wh = c.Wh, *bh = c.bh;
  const float *gamma = c.gamma, *dout = c.dout;
  const float eps = c.eps;
  float *dh = c.dh, *dagg = c.dagg, *dparams = c.dparams, *workspace = c.workspace, *saved = c.saved;
  const int32_t *ridx = c.row_index, *nrows_dev = c.n_rows;
  const int64_t rows = c.rows;
  const int D = c.D, accumulate = c.accumulate;
  const hipStream_t s = c.stream;
  const int R = kBlock / D;
  const int nblk = gu_main_blocks(rows, D), nchunk = gu_chunks(rows, D);
  int nsmall = nblk;  // slices of `small` the reduction reads
  // saved (impnn_gated_update_rows_train's buffer, [z | r | tanh(t)] then r * h): used in place of the workspace's
  // first two regions and CONSUMED - it leaves holding the pre-activation gradients
  float* dpre = saved ? saved : workspace;
  float* rh = dpre + rows * 3 * D;
  float* small = workspace + rows * 4 * D;
  float* gpart = small + (int64_t)nblk * 5 * D;
  float* wt = gpart + (int64_t)3 * nchunk * 2 * D * D;
  float* hc = ridx ? wt + (int64_t)3 * 2 * D * D : nullptr;  // compact copies of the listed rows (row-list form)
  float* aggc = ridx ? hc + rows * D : nullptr;
  size_t lds = sizeof(float) * ((size_t)10 * R * D + 4 * R);
  if (lds < sizeof(float) * 5 * kBlock) lds = sizeof(float) * 5 * kBlock;
  const size_t wlds = sizeof(float) * (size_t)3 * 2 * D * (D + 1);
  const bool al16 = ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(agg) | reinterpret_cast<uintptr_t>(dout) |
                      reinterpret_cast<uintptr_t>(dh) | reinterpret_cast<uintptr_t>(dagg) |
                      reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(dpre)) & 15u) == 0;
  if ((D == 64 || D == 128) && al16) {
    const size_t lw = sizeof(float) * ((size_t)64 * (2 * D + 4) + 64 * (D + 4) + 3 * 16 * 2 * D + 4 * 256) + 64 * sizeof(int32_t);
    const int tile_rows = gu_wide_tile_rows(rows);  // (as the forward kernel: 16-row tiles below ~8 K rows)
    transpose3_kernel<<<dim3((D + 31) / 32, (2 * D + 31) / 32, 3), dim3(32, 8), 0, s>>>(Wz, Wr, Wh, wt, D);
    if (int rc = check_launch("transpose3")) return rc;
    const int64_t tiles64 = (rows + tile_rows - 1) / tile_rows;
    const int nb = (int)(tiles64 < nblk ? tiles64 : nblk);  // every launched workgroup writes its slice of `small`
    nsmall = nb;                                            // (zeros when the row list ends before its tiles)
#define BWD16(NT_, SV_)                                                                                              \
    do {                                                                                                              \
      (void)hipFuncSetAttribute((const void*)gated_update_bwd_wide16_kernel<NT_, SV_, Drop...>,                       \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lw);                                 \
      gated_update_bwd_wide16_kernel<NT_, SV_, Drop...><<<nb, 1024, lw, s>>>(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, eps, \
                                                                            dout, dh, dagg, dpre, rh, small, rows,    \
                                                                            ridx, nrows_dev, hc, aggc, tile_rows, wt, \
                                                                            drop...);                                 \
    } while (0)
    if (D == 64) {
      if (saved) BWD16(4, true); else BWD16(4, false);
    } else {
      if (saved) BWD16(8, true); else BWD16(8, false);
    }
#undef BWD16
  } else if (D == 32 && al16) {
    const size_t l32 = sizeof(float) * ((size_t)3 * 32 * kBwT + 3 * 64 * kBwN + 4 * 32 + 4 * 5 * 32);
    if (l32 > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)gated_update_bwd_d32_kernel<false, Drop...>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)l32);
    if (saved) {
      const size_t l32s = l32 - sizeof(float) * 3 * 32 * kBwT;  // no transposed kernels
      gated_update_bwd_d32_kernel<true, Drop...><<<nblk, kBlock, l32s, s>>>(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, eps, dout,
                                                                          dh, dagg, dpre, rh, small, rows, drop...);
    } else {
      gated_update_bwd_d32_kernel<false, Drop...><<<nblk, kBlock, l32, s>>>(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, eps, dout,
                                                                           dh, dagg, dpre, rh, small, rows, drop...);
    }
  } else if (lds + wlds <= 120 * 1024) {
    lds += wlds;
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)gated_update_bwd_kernel<true, kBlock, Drop...>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    gated_update_bwd_kernel<true, kBlock, Drop...><<<nblk, kBlock, lds, s>>>(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, eps, dout,
                                                                             dh, dagg, dpre, rh, small, nullptr, rows, D, R,
                                                                             drop...);
  } else {
    constexpr int kBig = 1024;
    const int Rb = kBig / D;
    size_t lb = sizeof(float) * ((size_t)10 * Rb * D + 4 * Rb);
    if (lb < sizeof(float) * 5 * kBig) lb = sizeof(float) * 5 * kBig;
    if (lb > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)gated_update_bwd_kernel<false, kBig, Drop...>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    transpose3_kernel<<<dim3((D + 31) / 32, (2 * D + 31) / 32, 3), dim3(32, 8), 0, s>>>(Wz, Wr, Wh, wt, D);
    if (int rc = check_launch("transpose3")) return rc;
    gated_update_bwd_kernel<false, kBig, Drop...><<<nblk, kBig, lb, s>>>(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, eps, dout, dh,
                                                                         dagg, dpre, rh, small, wt, rows, D, Rb, drop...);
  }
  if (int rc = check_launch("gated_update_bwd")) return rc;
  int tiles_n = 1;
  const int tiles = gu_tiles(D, rows, &tiles_n);
  GemmProblems ga;
  const float* gh = ridx ? hc : h;      // the GEMMs contract over the listed rows: their compact copies
  const float* ga_ = ridx ? aggc : agg;
  ga.A1[0] = gh; ga.A2[0] = ga_; ga.B[0] = dpre;
  ga.A1[1] = gh; ga.A2[1] = ga_; ga.B[1] = dpre + D;
  ga.A1[2] = rh; ga.A2[2] = ga_; ga.B[2] = dpre + 2 * D;
  const bool al16g = ((reinterpret_cast<uintptr_t>(gh) | reinterpret_cast<uintptr_t>(ga_) | reinterpret_cast<uintptr_t>(rh) |
                       reinterpret_cast<uintptr_t>(dpre)) & 15u) == 0;
  if (gu_big_tiles(D, rows) && al16g)
    strided_gemm_splitk_big_kernel<<<dim3(nchunk, tiles, 3), kBlock, 0, s>>>(ga, gpart, rows, 2 * D, D, D, D, 3 * D, nchunk,
                                                                             tiles_n, ridx ? nrows_dev : nullptr);
  else if (gu_big_tiles(D, rows))
    return fail(IMPNN_E_BADARG, "gated_update_bwd: tensors must be 16B aligned at atom_dim %d", D);
  else
    strided_gemm_splitk_kernel<<<dim3(nchunk, tiles, 3), kBlock, 0, s>>>(ga, gpart, rows, 2 * D, D, D, D, 1, 3 * D, 1,
                                                                         nchunk, tiles_n, ridx ? nrows_dev : nullptr);
  if (int rc = check_launch("strided_gemm_splitk")) return rc;
  const int64_t welems = (int64_t)3 * 2 * D * D * (nchunk <= 64 ? 1 : 64);  // a thread or a wave per kernel element
  const int wblocks = (int)((welems + kBlock - 1) / kBlock), vblocks = (5 * D * 64 + kBlock - 1) / kBlock;
  gated_update_reduce_kernel<<<wblocks + vblocks, kBlock, 0, s>>>(small, gpart, dparams, nsmall, nchunk, D, accumulate,
                                                                 wblocks);
  return check_launch("gated_update_reduce");
}

int launch_gated_update_bwd(const GatedUpdateCall& c) {
  // the dropout instantiations of the main kernel; the GEMMs and the reduction behind it are the same
  return with_dropout_pack(c, [&](auto... drop) { return launch_gated_update_bwd_impl(c, drop...); });
}

// impnn_dropout_step: snapshot <- counter; counter += 1 (one thread; a captured step replays it)
__global__ void dropout_step_kernel(long long* __restrict__ counter, long long* __restrict__ snapshot) {
  const long long v = *counter;
  *snapshot = v;
  *counter = v + 1;
}

int launch_dropout_step(int64_t* counter, int64_t* snapshot, hipStream_t s) {
  dropout_step_kernel<<<1, 1, 0, s>>>(reinterpret_cast<long long*>(counter), reinterpret_cast<long long*>(snapshot));
  return check_launch("dropout_step");
}

// impnn_dropout_mask: out[row, c] = scale or 0, the mask the GatedUpdate kernels apply (one thread per column quad)
__global__ void dropout_mask_kernel(DropoutArgs d, const int32_t* __restrict__ ridx, const int32_t* __restrict__ nrows_dev,
                                    int64_t max_rows, int D, float* __restrict__ out) {
  int64_t rows = max_rows;
  if (nrows_dev) {
    const int64_t n = *nrows_dev;
    rows = n < 0 ? 0 : (n < max_rows ? n : max_rows);
  }
  const DropoutKey dk = dropout_key(d);
  const int Q = (D + 3) / 4;
  const int64_t n = rows * Q;
  for (int64_t t4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t4 < n; t4 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t4 / Q;
    const int c4 = (int)(t4 - i * Q);
    int64_t row = ridx ? (int64_t)ridx[i] : i;
    if (row < 0 || row >= max_rows) continue;  // (indices are never trusted)
    const Philox4 bits = dropout_bits(dk, row, c4);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (4 * c4 + u < D) out[row * D + 4 * c4 + u] = dropout_apply(dk, bits.v[u], 1.0f);
  }
}

int launch_dropout_mask(const DropoutArgs& d, const int32_t* ridx, const int32_t* nrows_dev, int64_t max_rows, int D,
                        float* out, hipStream_t s) {
  const int64_t n = max_rows * ((D + 3) / 4);
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  dropout_mask_kernel<<<(unsigned)blocks, 256, 0, s>>>(d, ridx, nrows_dev, max_rows, D, out);
  return check_launch("dropout_mask");
}

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

int launch_bond_type_matrices_multi(const float* tb, const float* const* W, float* const* out, int n, int Vb, int K,
                                    int D, hipStream_t s) {
  const int DD = D * D;
  for (int p0 = 0; p0 < n; p0 += kBtmMax) {
    BtmBatch bt{};
    bt.n = n - p0 < kBtmMax ? n - p0 : kBtmMax;
    for (int q = 0; q < bt.n; ++q) {
      if (!W[p0 + q] || !out[p0 + q]) return fail(IMPNN_E_BADARG, "bond_type_matrices_multi: null tensor %d", p0 + q);
      bt.W[q] = W[p0 + q];
      bt.out[q] = out[p0 + q];
    }
    if (K <= kBtmSmallK && Vb * K <= kBtmTbMax && DD >= 4096)  // (small matrices: too few workgroups this way)
      bond_type_matrices_multi_smallk_kernel<<<dim3((DD + kBlock - 1) / kBlock, bt.n), kBlock, 0, s>>>(tb, bt, Vb, K, DD);
    else
      bond_type_matrices_multi_kernel<<<dim3((DD + kBlock - 1) / kBlock, Vb, bt.n), kBlock, 0, s>>>(tb, bt, Vb, K, DD);
    if (int rc = check_launch("bond_type_matrices_multi")) return rc;
  }
  return IMPNN_OK;
}

int64_t bond_type_matrices_multi_bwd_workspace(int n, int Vb, int K, int D) {
  const int nb = n < kBtmMax ? n : kBtmMax;
  return (int64_t)nb * ((int64_t)D * D / kBtC + 1) * Vb * K;
}

int launch_bond_type_matrices_multi_bwd(const float* tb, const float* const* W, const float* const* dA,
                                        float* const* dW, float* dtb, int n, int Vb, int K, int D, int accumulate,
                                        hipStream_t s, float* workspace) {
  const int DD = D * D;
  // with a workspace: the bond-table gradient on the matrix cores (partials per wave, summed in a fixed order)
  const bool mfma_t = workspace && K <= 16 && Vb <= 128 && DD % kBtC == 0 && DD >= 4096 &&  // (small matrices: one launch less)
                      (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0;
  for (int p0 = 0; p0 < n; p0 += kBtmMax) {
    BtmBatch bt{};
    bt.n = n - p0 < kBtmMax ? n - p0 : kBtmMax;
    for (int q = 0; q < bt.n; ++q) {
      if (!W[p0 + q] || !dA[p0 + q] || !dW[p0 + q])
        return fail(IMPNN_E_BADARG, "bond_type_matrices_multi_bwd: null tensor %d", p0 + q);
      bt.W[q] = W[p0 + q];
      bt.dA[q] = dA[p0 + q];
      bt.out[q] = dW[p0 + q];
    }
    bond_type_matrices_multi_bwd_w_kernel<<<dim3((DD + kBlock - 1) / kBlock, K, bt.n), kBlock, 0, s>>>(tb, bt, Vb, K, DD,
                                                                                                     accumulate);
    if (int rc = check_launch("bond_type_matrices_multi_bwd_w")) return rc;
    bool al = mfma_t;
    for (int q = 0; q < bt.n; ++q)
      al = al && ((reinterpret_cast<uintptr_t>(bt.W[q]) | reinterpret_cast<uintptr_t>(bt.dA[q])) & 15u) == 0;
    if (al) {
      const int nw = bt.n * (DD / kBtC), nwg = (nw + 3) / 4, acc_t = (accumulate || p0 > 0) ? 1 : 0;
      switch ((Vb + 15) / 16) {
#define BTM_T(VT_)                                                                                                  \
        case VT_:                                                                                                     \
          bond_type_matrices_multi_bwd_t_mfma_kernel<VT_><<<nwg, 256, 0, s>>>(bt, workspace, Vb, K, DD, nw);          \
          break;
        BTM_T(1) BTM_T(2) BTM_T(3) BTM_T(4) BTM_T(5) BTM_T(6) BTM_T(7) BTM_T(8)
#undef BTM_T
      }
      if (int rc = check_launch("bond_type_matrices_multi_bwd_t_mfma")) return rc;
      bond_type_matrices_t_sum_kernel<<<(Vb * K * 64 + kBlock - 1) / kBlock, kBlock, 0, s>>>(workspace, dtb, Vb * K, nw,
                                                                                           acc_t);
      if (int rc = check_launch("bond_type_matrices_t_sum")) return rc;
      continue;
    }
    const int64_t waves = (int64_t)Vb * K;
    // (tried for bond_dim <= 8: one workgroup per bond type with the K partial dot products per thread, dA read once
    //  instead of once per k - 71 workgroups are far too few: 116 us -> 1.3 ms at atom_dim 128)
    bond_type_matrices_multi_bwd_t_kernel<<<(int)((waves * 64 + kBlock - 1) / kBlock), kBlock, 0, s>>>(
        bt, dtb, Vb, K, DD, (accumulate || p0 > 0) ? 1 : 0);
    if (int rc = check_launch("bond_type_matrices_multi_bwd_t")) return rc;
  }
  return IMPNN_OK;
}

}  // namespace impnn
