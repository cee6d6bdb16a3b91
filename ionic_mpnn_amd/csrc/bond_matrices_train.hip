// The bond-type matrices in training (schedule A): A[v] = sum_k Tb[v,k] W[k], the per-bond-type
// matrices that replace the reference's per-edge Dense of the bond state (models/layers.py:114-115).  Holds the adjoint
// of layer_kernels.hip's bond_type_matrices (dW, dTb) for one message layer, and for ALL message layers of a model in
// one launch each: a training-time forward and its backward, the latter also on the matrix cores.  Written for any D
// (f32).  Every sum runs in a fixed order - vocabulary order, problems then lanes, or per-wave partials that a second
// kernel adds in wave order - so the gradients are bitwise reproducible.  K >= 64 goes through launch_strided_gemm
// (gated_update_bwd.hip).
#include "kernel_device.h"

namespace impnn {
namespace {

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

}  // namespace

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
