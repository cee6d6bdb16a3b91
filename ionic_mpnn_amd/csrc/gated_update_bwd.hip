// The GatedUpdate backward: what Keras autodiff does for the reference's GatedUpdate layer (a7,
// models/layers.py:142-156), the adjoint of the forward in layer_kernels.hip with the same dropout mask.  A main kernel
// per row tile (generic VALU for any D, one for atom_dim 32, a matrix-core one for 64 / 128), split-K GEMMs for the
// three kernel gradients, and a reduction: the parameter-gradient sums run over per-workgroup and per-chunk partial
// buffers that the reduction adds in a fixed order, so they are bitwise reproducible.  GuBwdPlan lays the workspace
// out, choose_gu_bwd picks the main kernel.  The message adjoint (a4) is in message_typed.hip, the model head's
// backward in model_head.hip.
#include "kernel_device.h"

namespace impnn {
namespace {

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }

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

}  // namespace

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

int64_t gated_update_param_floats(int D) { return 3 * ((int64_t)2 * D * D + D) + 2 * D; }

// The launch sizes of a backward over `rows` rows and the workspace they fix, as float offsets:
//   dpre rows*3D | rh (r*h) rows*D | small nblk*5D | gpart (GEMM partials) 3*nchunk*2D*D | wt (W^T) 3*2D*D
//   | hc, aggc (compact copies of the listed rows' h and agg) rows*D each: row-list form only, -1 without
struct GuBwdPlan {
  int nblk, nchunk, tiles, tiles_n;  // main-kernel workgroups; row chunks, output tiles (and tiles along N) of the GEMMs
  bool big_tiles;
  int64_t dpre, rh, small, gpart, wt, hc, aggc, total;
};
static GuBwdPlan gu_bwd_plan(int64_t rows, int D, bool row_list) {
  GuBwdPlan p;
  // tiles of the main kernel: kBlock / D rows (generic kernels), 16 or 64 rows (the wide matrix-core kernel)
  const int R = (D == 64 || D == 128) ? gu_wide_tile_rows(rows) : kBlock / D;
  p.nblk = (int)std::min<int64_t>(std::max<int64_t>((rows + R - 1) / R, 1), 1024);
  // 128 x 64 output tiles: atom_dim 64 / 128 from 8 K rows (below that the 64 x 32 tiles give 4x the workgroups: 1.445
  // vs 1.478 ms per step at batch 32)
  p.big_tiles = D % kBN == 0 && (2 * D) % kBM == 0 && rows >= 8192;
  const int gn = p.big_tiles ? kBN : kGN, gm = p.big_tiles ? kBM : kGM;
  p.tiles_n = (D + gn - 1) / gn;
  p.tiles = (2 * D + gm - 1) / gm * p.tiles_n;
  // ~1024 workgroups of the 64 x 32 tiles, ~768 (three resident per CU) of the 128 x 64 ones; at least 256 contraction
  // rows per chunk: fewer partials to write and add
  const int64_t want = ((p.big_tiles ? 768 : 1024) + 3 * p.tiles - 1) / (3 * p.tiles);
  p.nchunk = (int)std::max<int64_t>(std::min<int64_t>(want, (rows + 255) / 256), 1);
  const int64_t W3 = (int64_t)3 * 2 * D * D;
  p.dpre = 0;
  p.rh = p.dpre + rows * 3 * D;
  p.small = p.rh + rows * D;
  p.gpart = p.small + (int64_t)p.nblk * 5 * D;
  p.wt = p.gpart + p.nchunk * W3;
  p.hc = row_list ? p.wt + W3 : -1;
  p.aggc = row_list ? p.hc + rows * D : -1;
  p.total = row_list ? p.aggc + rows * D : p.wt + W3;
  return p;
}

int64_t gated_update_bwd_workspace(int64_t rows, int D, bool row_list) { return gu_bwd_plan(rows, D, row_list).total; }

// The main kernel of a backward.  al16: every tensor the kernel reads or writes is 16-byte aligned.
enum class GuBwdRoute {
  wide16,       // atom_dim 64 / 128 on the matrix cores
  d32,          // atom_dim 32 on the matrix cores
  generic_lds,  // any atom_dim, the gate kernels in LDS
  generic_wt    // any atom_dim, 1024 threads, the transposed kernels in global memory
};
struct GuBwdChoice {
  GuBwdRoute route;
  int block, tile_rows;
  size_t lds;      // dynamic LDS bytes
  bool transpose;  // transpose3 fills wt first
  int grid;        // workgroups, each of which writes its slice of `small`: the slices the reduction reads
};
static GuBwdChoice choose_gu_bwd(int D, int64_t rows, bool al16, bool saved) {
  constexpr size_t F = sizeof(float);
  const int nblk = gu_bwd_plan(rows, D, false).nblk;
  if ((D == 64 || D == 128) && al16) {
    const int tr = gu_wide_tile_rows(rows);  // (as the forward kernel: 16-row tiles below ~8 K rows)
    const size_t lw = F * (64 * (2 * D + 4) + 64 * (D + 4) + 3 * 16 * 2 * D + 4 * 256) + 64 * sizeof(int32_t);
    // (a workgroup whose tiles lie past the end of the row list writes zeros)
    return {GuBwdRoute::wide16, 1024, tr, lw, true, (int)std::min<int64_t>((rows + tr - 1) / tr, nblk)};
  }
  if (D == 32 && al16)  // saved: no transposed kernels in LDS
    return {GuBwdRoute::d32, kBlock, 16, F * ((saved ? 0 : 3 * 32 * kBwT) + 3 * 64 * kBwN + 4 * 32 + 4 * 5 * 32),
            false, nblk};
  // ten R x D tiles and 4 R row statistics, R = block / D; the closing column sums take 5 floats per thread
  const auto tiles_lds = [D](int block) { return F * std::max(10 * (block / D) * D + 4 * (block / D), 5 * block); };
  const size_t lds = tiles_lds(kBlock) + F * 3 * 2 * D * (D + 1);  // + the three gate kernels, row stride D + 1
  if (lds <= 120 * 1024) return {GuBwdRoute::generic_lds, kBlock, kBlock / D, lds, false, nblk};
  return {GuBwdRoute::generic_wt, 1024, 1024 / D, tiles_lds(1024), true, nblk};
}

// (api.hip has checked the call: atom_dim divides 256, and a row list or a `saved` buffer comes with an atom_dim and
// alignment it covers)
template <class... Drop>
static int launch_gated_update_bwd_impl(const GatedUpdateCall& c, Drop... drop) {
  const int64_t rows = c.rows;
  const int D = c.D;
  const hipStream_t s = c.stream;
  const int32_t *ridx = c.row_index, *nrows_dev = c.n_rows;
  const GuBwdPlan p = gu_bwd_plan(rows, D, ridx != nullptr);
  // saved (impnn_gated_update_rows_train's buffer, [z | r | tanh(t)] then r * h): used in place of the workspace's
  // first two regions and CONSUMED - it leaves holding the pre-activation gradients
  float *ws = c.workspace, *front = c.saved ? c.saved : ws;
  float *dpre = front + p.dpre, *rh = front + p.rh, *small = ws + p.small, *gpart = ws + p.gpart, *wt = ws + p.wt;
  float *hc = ridx ? ws + p.hc : nullptr, *aggc = ridx ? ws + p.aggc : nullptr;
  const auto bits = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  const bool al16 =
      ((bits(c.h) | bits(c.agg) | bits(c.dout) | bits(c.dh) | bits(c.dagg) | bits(ws) | bits(dpre)) & 15u) == 0;
  const GuBwdChoice ch = choose_gu_bwd(D, rows, al16, c.saved != nullptr);
  if (ch.transpose) {
    transpose3_kernel<<<dim3((D + 31) / 32, (2 * D + 31) / 32, 3), dim3(32, 8), 0, s>>>(c.Wz, c.Wr, c.Wh, wt, D);
    if (int rc = check_launch("transpose3")) return rc;
  }
  // every main kernel opens with the same sixteen operands and closes with the dropout pack
  const auto run = [&](auto kernel, auto... tail) {
    if (ch.lds > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ch.lds);
    kernel<<<ch.grid, ch.block, ch.lds, s>>>(c.h, c.agg, c.Wz, c.bz, c.Wr, c.br, c.Wh, c.bh, c.gamma, c.eps, c.dout, c.dh,
                                              c.dagg, dpre, rh, small, tail..., drop...);
  };
  const auto wide = [&](auto kernel) { run(kernel, rows, ridx, nrows_dev, hc, aggc, ch.tile_rows, (const float*)wt); };
  switch (ch.route) {
    case GuBwdRoute::wide16:
      if (D == 64 && c.saved) wide(gated_update_bwd_wide16_kernel<4, true, Drop...>);
      else if (D == 64) wide(gated_update_bwd_wide16_kernel<4, false, Drop...>);
      else if (c.saved) wide(gated_update_bwd_wide16_kernel<8, true, Drop...>);
      else wide(gated_update_bwd_wide16_kernel<8, false, Drop...>);
      break;
    case GuBwdRoute::d32:
      if (c.saved) run(gated_update_bwd_d32_kernel<true, Drop...>, rows);
      else run(gated_update_bwd_d32_kernel<false, Drop...>, rows);
      break;
    case GuBwdRoute::generic_lds:
      run(gated_update_bwd_kernel<true, kBlock, Drop...>, (const float*)nullptr, rows, D, ch.tile_rows);
      break;
    case GuBwdRoute::generic_wt:
      run(gated_update_bwd_kernel<false, 1024, Drop...>, (const float*)wt, rows, D, ch.tile_rows);
      break;
  }
  if (int rc = check_launch("gated_update_bwd")) return rc;
  GemmProblems ga;
  const float* gh = ridx ? hc : c.h;      // the GEMMs contract over the listed rows: their compact copies
  const float* ga_ = ridx ? aggc : c.agg;
  ga.A1[0] = gh; ga.A2[0] = ga_; ga.B[0] = dpre;
  ga.A1[1] = gh; ga.A2[1] = ga_; ga.B[1] = dpre + D;
  ga.A1[2] = rh; ga.A2[2] = ga_; ga.B[2] = dpre + 2 * D;
  const dim3 ggrid(p.nchunk, p.tiles, 3);
  if (p.big_tiles && ((bits(gh) | bits(ga_) | bits(rh) | bits(dpre)) & 15u) != 0)
    return fail(IMPNN_E_BADARG, "gated_update_bwd: tensors must be 16B aligned at atom_dim %d", D);
  if (p.big_tiles)
    strided_gemm_splitk_big_kernel<<<ggrid, kBlock, 0, s>>>(ga, gpart, rows, 2 * D, D, D, D, 3 * D, p.nchunk, p.tiles_n,
                                                            ridx ? nrows_dev : nullptr);
  else
    strided_gemm_splitk_kernel<<<ggrid, kBlock, 0, s>>>(ga, gpart, rows, 2 * D, D, D, D, 1, 3 * D, 1, p.nchunk, p.tiles_n,
                                                        ridx ? nrows_dev : nullptr);
  if (int rc = check_launch("strided_gemm_splitk")) return rc;
  const int64_t welems = (int64_t)3 * 2 * D * D * (p.nchunk <= 64 ? 1 : 64);  // a thread or a wave per kernel element
  const int wblocks = (int)((welems + kBlock - 1) / kBlock), vblocks = (5 * D * 64 + kBlock - 1) / kBlock;
  gated_update_reduce_kernel<<<wblocks + vblocks, kBlock, 0, s>>>(small, gpart, c.dparams, ch.grid, p.nchunk, D,
                                                                 c.accumulate, wblocks);
  return check_launch("gated_update_reduce");
}

int launch_gated_update_bwd(const GatedUpdateCall& c) {
  // the dropout instantiations of the main kernel; the GEMMs and the reduction behind it are the same
  return with_dropout_pack(c, [&](auto... drop) { return launch_gated_update_bwd_impl(c, drop...); });
}

}  // namespace impnn
