// f1 over a Cartesian product (include/impnn.h: impnn_head_ion_mix, impnn_head_grid).
//
// An ion's branch of the head never sees its partner until AddTwoTensors / Add (train_viscosity.py:189,197-201;
// train_melting_point.py:173,191), so a screen of C cations x A anions needs C + A mixing rows, not C * A:
//   head_ion_mix_kernel   mix_g[m] = relu(relu(pooled_g[m] Wfp_g + bfp_g) Wp_g + bp_g)      one row per ion species
//   head_grid_kernel      per pair (i, j): mixed = mix_cat[i] + mix_an[j], then the tail of model_head_kernel
// Every rounding step is the one of model_head_kernel (head_device.h; the same fmaf chains, bias first, inputs
// ascending), so element (i, j, t) carries the bits impnn_model_head gives for the sample (pooled_cat[i],
// pooled_an[j], T[t]).  No atomics, every sum in a fixed order.
#include "common.h"
#include "head_device.h"

namespace impnn {

namespace {

constexpr int kMixRows = 8;   // ion rows per 256-thread workgroup, 32 threads per row (as model_head_kernel)

__global__ __launch_bounds__(256) void head_ion_mix_kernel(const float* __restrict__ pooled,
                                                           const float* __restrict__ wfp_g,
                                                           const float* __restrict__ wp_g, float* __restrict__ mix,
                                                           int M, int D, int F, int Mx) {
  extern __shared__ __align__(16) float sm[];
  const int nfp = D * F + F, np = F * Mx + Mx;
  float* Wfp = sm;                          // Wfp_g D*F | bfp_g F
  float* Wp = Wfp + ((nfp + 3) & ~3);       // Wp_g F*Mx | bp_g Mx
  float* xs = Wp + ((np + 3) & ~3);         // [kMixRows][kHeadMaxX]
  float* fp = xs + kMixRows * kHeadMaxX;        // [kMixRows][kHeadMaxDim]
  const int tid = threadIdx.x, sl = tid >> 5, jj = tid & 31;
  const int64_t m = (int64_t)blockIdx.x * kMixRows + sl;
  const bool live = m < M;
  for (int t = tid; t < nfp; t += blockDim.x) Wfp[t] = wfp_g[t];
  for (int t = tid; t < np; t += blockDim.x) Wp[t] = wp_g[t];
  for (int i = jj; i < D; i += 32) xs[sl * kHeadMaxX + i] = live ? pooled[m * D + i] : 0.f;
  __syncthreads();
  for (int j = jj; j < F; j += 32)
    fp[sl * kHeadMaxDim + j] = head_relu(head_chain(xs + sl * kHeadMaxX, Wfp + j, F, D, Wfp[D * F + j]));
  __syncthreads();
  if (live)
    for (int j = jj; j < Mx; j += 32)
      mix[m * Mx + j] = head_relu(head_chain(fp + sl * kHeadMaxDim, Wp + j, Mx, F, Wp[F * Mx + j]));
}

// ---- the grid.  One workgroup owns kTileC cations x kTileA anions; lane = anion, a wave walks the tile's cations.
constexpr int kTileC = 16, kTileA = 64, kTilePairs = kTileC * kTileA;
constexpr int kGridMaxT = 4096;  // temperatures per launch: T / 100 sits in LDS (16 KB)

// Row stride (floats) of the mixing rows in LDS.  A lane reads its anion's row 16 bytes at a time (ds_read_b128: 16
// lanes per LDS cycle, 64 banks), so the 16 lanes of a group must start 4 banks apart: stride = 4 * odd.  Mx = 64
// unpadded would put all 64 lanes on one bank quad; the default Mx = 20 is 4 * 5 already.
__host__ __device__ inline int mix_row_stride(int Mx) {
  const int s = (Mx + 3) & ~3;
  return ((s >> 2) & 1) ? s : s + 4;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

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

// KIND 0: MXR unused (0).  KIND 1: MXR = 32 or 64 registers hold a pair's mixed vector.
template <int KIND, int MXR>
__global__ __launch_bounds__(256) void head_grid_kernel(const float* __restrict__ mix_cat,
                                                        const float* __restrict__ mix_an,
                                                        const float* __restrict__ T, const float* __restrict__ tail,
                                                        float* __restrict__ out, float* __restrict__ params, int C,
                                                        int A, int nT, int F, int Mx, int tiles_a) {
  extern __shared__ __align__(16) float sm[];
  const int S = mix_row_stride(Mx);
  float* man = sm;                     // [kTileA][S]
  float* mcat = man + kTileA * S;      // [kTileC][S]
  float* wts = mcat + kTileC * S;      // the tail weights
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = (blockIdx.x / tiles_a) * kTileC, a0 = (blockIdx.x % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);

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
    store_rows(out, ((int64_t)c0 * A + a0) * nT, (int64_t)A * nT, nc, na * nT, nT, [&](int r, int a, int t) {
      return head_vft_eval(VftParams{resA[r * kTileA + a], resB[r * kTileA + a], resC[r * kTileA + a]}, t100[t]);
    });
    if (params)
      store_rows(params, ((int64_t)c0 * A + a0) * 3, (int64_t)A * 3, nc, na * 3, 3, [&](int r, int a, int t) {
        return (t == 0 ? resA : t == 1 ? resB : resC)[r * kTileA + a];
      });
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
    store_rows(out, (int64_t)c0 * A + a0, (int64_t)A, nc, na, 1, [&](int r, int a, int) { return res[r * kTileA + a]; });
  }
}

size_t grid_lds_floats(int kind, int nT, int F, int Mx) {
  const size_t rows = (size_t)(kTileA + kTileC) * mix_row_stride(Mx);
  if (kind == 0) return rows + align4((size_t)Mx * 3 + 3) + 3 * (size_t)kTilePairs + align4((size_t)nT);
  return rows + (size_t)F * align4(Mx) + align4(F) + align4((size_t)F + 1) + kTilePairs;
}

}  // namespace

int launch_head_ion_mix(int kind, int ion, const float* pooled, const float* w, float* mix, int M, int D, int F, int Mx,
                        hipStream_t s) {
  (void)kind;  // both kinds share the per-ion layout
  const int nfp = D * F + F, np = F * Mx + Mx;
  const size_t lds = sizeof(float) * (align4(nfp) + align4(np) + (size_t)kMixRows * (kHeadMaxX + kHeadMaxDim));  // <= 54.3 KiB
  head_ion_mix_kernel<<<(int)(((int64_t)M + kMixRows - 1) / kMixRows), 256, lds, s>>>(pooled, w + (size_t)ion * nfp,
                                                                      w + 2 * (size_t)nfp + (size_t)ion * np, mix, M, D, F, Mx);
  return check_launch("head_ion_mix");
}

int head_grid_max_temperatures() { return kGridMaxT; }

int launch_head_grid(int kind, const float* mix_cat, const float* mix_an, const float* T, const float* w, float* out,
                     float* params, int C, int A, int nT, int D, int F, int Mx, hipStream_t s) {
  const int tiles_a = (A + kTileA - 1) / kTileA;
  const int64_t tiles = (int64_t)((C + kTileC - 1) / kTileC) * tiles_a;
  if (tiles > 0x7fffffff)
    return fail(IMPNN_E_UNSUPPORTED, "head_grid: %lld tiles of %d x %d pairs exceed one launch; split the cation axis",
                (long long)tiles, kTileC, kTileA);
  const float* tail = w + 2 * ((size_t)D * F + F) + 2 * ((size_t)F * Mx + Mx);
  const size_t lds = sizeof(float) * grid_lds_floats(kind, nT, F, Mx);  // <= 50.0 KiB (kind 0), 41.8 KiB (kind 1)
  if (kind == 0)
    head_grid_kernel<0, 0><<<(int)tiles, 256, lds, s>>>(mix_cat, mix_an, T, tail, out, params, C, A, nT, F, Mx, tiles_a);
  else if (Mx <= 32)
    head_grid_kernel<1, 32><<<(int)tiles, 256, lds, s>>>(mix_cat, mix_an, T, tail, out, params, C, A, nT, F, Mx, tiles_a);
  else
    head_grid_kernel<1, 64><<<(int)tiles, 256, lds, s>>>(mix_cat, mix_an, T, tail, out, params, C, A, nT, F, Mx, tiles_a);
  return check_launch("head_grid");
}

}  // namespace impnn
