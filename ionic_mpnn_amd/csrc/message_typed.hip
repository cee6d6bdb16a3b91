// The typed-message family (a4 in the per-bond-type schedule): the counting sort of a batch's valid edges by bond
// type, the forward over the sorted segments (the inference path of every atom_dim other than 32, and of training)
// and the message adjoint, VALU for any D <= 128 and on the matrix cores for D = 64 / 128.  The entries of
// include/impnn.h that end here (impnn_bmm_message_typed_sorted, impnn_bmm_message_typed_bwd,
// impnn_message_reduce_typed_bwd[_scratch]) fill a TypedMessageCall, which api.hip checks before it launches.
#include <cstdlib>

#include "kernel_device.h"

namespace impnn {
namespace {

// ---------------------------------------------------------------------------------------
// a4 backward in the per-bond-type schedule.  Forward: m[b,e,:] = A[type_e] h[b,src_e,:] on valid edges.
//   dh[b,src,:]  += A[type]^T dm[b,e,:]
//   dA[type,i,j] += dm[b,e,i] h[b,src,j]
// The valid edges of the WHOLE batch are counting-sorted by bond type (histogram, prefix, scatter - three
// small launches), and every workgroup of the main kernel takes one segment of <= kSeg edges of one type:
// A[type] and the segment's dm / h rows are staged in LDS, dA of the segment is summed in registers ((i,j)
// entries dealt over the threads) and leaves with one atomicAdd per entry, dh goes out with float atomics
// (several edges share a source row).  Parallelism is edges/kSeg workgroups at any batch size (a batch of
// 32 molecules still gives ~100).  dh and dA must be zeroed by the caller.
// workspace (int32, EdgeSortView in common.h): cnt Vb+1 | start Vb+1 | cursor Vb+1 | segbase Vb+1 | order B*E
// ---------------------------------------------------------------------------------------
constexpr int kSeg = 64;  // (kMaxTypes: common.h, beside TypedMessageCall)

__device__ __forceinline__ int edge_type_or_neg(const int32_t* conn, const int32_t* bond_ids, int64_t be, int N, int Vb) {
  const int src = conn[be * 2], tgt = conn[be * 2 + 1], ty = bond_ids[be];
  return (src > 0 && tgt > 0 && src < N && tgt < N && (unsigned)ty < (unsigned)Vb) ? ty : -1;
}

__global__ void zero_ints_kernel(int32_t* __restrict__ p, int n) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) p[t] = 0;
}

// Histogram of the valid edges by type.  Each workgroup counts a contiguous slice in LDS first and touches the
// global counters once per type it saw: with ~10^2 types and ~10^5 edges, per-edge global atomics serialise.
__global__ __launch_bounds__(kBlock) void edge_type_hist_kernel(const int32_t* __restrict__ conn,
                                                                const int32_t* __restrict__ bond_ids,
                                                                int32_t* __restrict__ cnt, int64_t BE, int N, int Vb) {
  __shared__ int32_t lh[kMaxTypes];
  for (int t = threadIdx.x; t < Vb; t += kBlock) lh[t] = 0;
  __syncthreads();
  const int64_t per = (BE + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < BE ? lo + per : BE;
  for (int64_t be = lo + threadIdx.x; be < hi; be += kBlock) {
    const int ty = edge_type_or_neg(conn, bond_ids, be, N, Vb);
    if (ty >= 0) atomicAdd(&lh[ty], 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Vb; t += kBlock)
    if (lh[t]) atomicAdd(&cnt[t], lh[t]);
}

// one workgroup: start[t] = exclusive prefix of cnt, cursor = start, segbase[t] = exclusive prefix of
// ceil(cnt[t] / kSeg); start[Vb] = valid edges, segbase[Vb] = segments
__global__ void edge_type_prefix_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ start,
                                        int32_t* __restrict__ cursor, int32_t* __restrict__ segbase, int Vb) {
  if (threadIdx.x == 0) {
    int run = 0, segs = 0;
    for (int t = 0; t < Vb; ++t) {
      const int c = cnt[t];
      start[t] = run;
      cursor[t] = run;
      segbase[t] = segs;
      run += c;
      segs += (c + kSeg - 1) / kSeg;
    }
    start[Vb] = run;
    segbase[Vb] = segs;
  }
}

// Scatter of the valid edges into their type's run: a workgroup counts its slice in LDS, reserves one range per type
// with a single global atomic, and places its edges inside the reserved ranges with LDS atomics.
__global__ __launch_bounds__(kBlock) void edge_type_scatter_kernel(const int32_t* __restrict__ conn,
                                                                   const int32_t* __restrict__ bond_ids,
                                                                   int32_t* __restrict__ cursor,
                                                                   int32_t* __restrict__ order, int64_t BE, int N,
                                                                   int Vb) {
  __shared__ int32_t lh[kMaxTypes];  // count, then the next free position of the reserved range
  for (int t = threadIdx.x; t < Vb; t += kBlock) lh[t] = 0;
  __syncthreads();
  const int64_t per = (BE + gridDim.x - 1) / gridDim.x;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < BE ? lo + per : BE;
  for (int64_t be = lo + threadIdx.x; be < hi; be += kBlock) {
    const int ty = edge_type_or_neg(conn, bond_ids, be, N, Vb);
    if (ty >= 0) atomicAdd(&lh[ty], 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Vb; t += kBlock) {
    const int c = lh[t];
    lh[t] = c ? atomicAdd(&cursor[t], c) : 0;
  }
  __syncthreads();
  for (int64_t be = lo + threadIdx.x; be < hi; be += kBlock) {
    const int ty = edge_type_or_neg(conn, bond_ids, be, N, Vb);
    if (ty >= 0) order[atomicAdd(&lh[ty], 1)] = (int32_t)be;
  }
}

// The whole sort in ONE workgroup for small batches (the reference trains with 32 pairs: 8 K edge slots): every
// thread keeps the types of its <= 16 slots in registers between the histogram and the scatter, the scan over the
// types runs one type per thread.  Replaces four launches (zero, hist, prefix, scatter).
constexpr int kSortSmallPer = 16;
__global__ __launch_bounds__(1024) void edge_type_sort_small_kernel(const int32_t* __restrict__ conn,
                                                                    const int32_t* __restrict__ bond_ids,
                                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ start,
                                                                    int32_t* __restrict__ cursor,
                                                                    int32_t* __restrict__ segbase,
                                                                    int32_t* __restrict__ order, int BE, int N, int Vb) {
  __shared__ int32_t lh[1024];  // counts, then the next free position of every type's run
  __shared__ int32_t wc[16], wsg[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  lh[tid] = 0;
  __syncthreads();
  int ty[kSortSmallPer];
#pragma unroll
  for (int u = 0; u < kSortSmallPer; ++u) {
    const int be = tid + u * 1024;
    ty[u] = be < BE ? edge_type_or_neg(conn, bond_ids, be, N, Vb) : -1;
  }
#pragma unroll
  for (int u = 0; u < kSortSmallPer; ++u)
    if (ty[u] >= 0) atomicAdd(&lh[ty[u]], 1);
  __syncthreads();
  const int c = tid < Vb ? lh[tid] : 0;
  const int sg = (c + kSeg - 1) / kSeg;
  int ic = c, is = sg;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int uc = __shfl_up(ic, o), us = __shfl_up(is, o);
    if (lane >= o) {
      ic += uc;
      is += us;
    }
  }
  if (lane == 63) {
    wc[wave] = ic;
    wsg[wave] = is;
  }
  __syncthreads();
  int oc = 0, os = 0;
  for (int w = 0; w < wave; ++w) {
    oc += wc[w];
    os += wsg[w];
  }
  ic += oc;
  is += os;
  if (tid < Vb) {
    cnt[tid] = c;
    start[tid] = ic - c;
    cursor[tid] = ic - c;
    segbase[tid] = is - sg;
    lh[tid] = ic - c;
  }
  if (tid == 1023) {  // threads past Vb carry zeros: the last inclusive value is the total
    start[Vb] = ic;
    segbase[Vb] = is;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kSortSmallPer; ++u)
    if (ty[u] >= 0) order[atomicAdd(&lh[ty[u]], 1)] = tid + u * 1024;
}

template <int ACC>  // ACC = ceil(D*D / blockDim.x) accumulators per thread
__global__ __launch_bounds__(1024) void bmm_message_typed_bwd_kernel(
    const float* __restrict__ h, const int32_t* __restrict__ conn, const float* __restrict__ A,
    const float* __restrict__ dm, float* __restrict__ dh, float* __restrict__ dA, const int32_t* __restrict__ start,
    const int32_t* __restrict__ segbase, const int32_t* __restrict__ order, int N, int E, int D, int Vb,
    int from_agg, float* __restrict__ du) {  // from_agg: dm is the gradient of Reduce's output (B,N,D) and dm of edge e is its row tgt(e)
  // du (optional): per-edge vectors to their edge slot's row instead of atomics on dh (see the matrix-core kernel below)
  extern __shared__ __align__(16) float smem[];
  __shared__ int64_t srcrow[kSeg];
  __shared__ int64_t slot[kSeg];
  const int seg = blockIdx.x;
  if (seg >= segbase[Vb]) return;  // the grid is an upper bound on the number of segments
  int lo = 0, hi = Vb - 1;          // type of this segment: largest t with segbase[t] <= seg
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segbase[mid] <= seg) lo = mid; else hi = mid - 1;
  }
  const int ty = lo;
  const int p0 = start[ty] + (seg - segbase[ty]) * kSeg;
  const int n = min(kSeg, start[ty + 1] - p0);
  if (n <= 0) return;
  const int tid = threadIdx.x;
  const int DD = D * D;
  float* As = smem;            // D*D
  float* gm = As + DD;         // kSeg x D: dm rows of the segment's edges
  float* xm = gm + kSeg * D;   // kSeg x D: their source rows of h
  for (int t = tid; t < DD; t += (int)blockDim.x) As[t] = A[(int64_t)ty * DD + t];
  for (int t = tid; t < n * D; t += (int)blockDim.x) {
    const int e = t / D, c = t - e * D;
    const int64_t be = order[p0 + e];
    const int64_t row = (be / E) * N + conn[be * 2];
    const int64_t grow = from_agg ? (be / E) * N + conn[be * 2 + 1] : be;
    gm[e * D + c] = dm[grow * D + c];
    xm[e * D + c] = h[row * D + c];
    if (c == 0) {
      srcrow[e] = row;
      slot[e] = be;
    }
  }
  __syncthreads();
  const int lanes = (int)blockDim.x / D > 0 ? (int)blockDim.x / D : 1;
  if (tid < lanes * D) {  // dh: thread (edge lane, column j)
    const int j = tid % D, el = tid / D;
    for (int e = el; e < n; e += lanes) {
      float u = 0.f;
      for (int i = 0; i < D; ++i) u = fmaf(gm[e * D + i], As[i * D + j], u);
      if (du) du[slot[e] * D + j] = u;
      else atomicAdd(&dh[srcrow[e] * D + j], u);
    }
  }
#pragma unroll
  for (int a = 0; a < ACC; ++a) {  // dA of this segment: entry q = (i, j)
    const int q = tid + a * (int)blockDim.x;
    if (q < DD) {
      const int i = q / D, j = q - i * D;
      float v = 0.f;
      for (int e = 0; e < n; ++e) v = fmaf(gm[e * D + i], xm[e * D + j], v);
      atomicAdd(&dA[(int64_t)ty * DD + q], v);
    }
  }
}

// ---------------------------------------------------------------------------------------
// The same adjoint on the matrix cores for wide states (D = 64, 128; exact f32 products).  Per 64-edge segment two
// GEMMs: dh rows = G A_t (features on M from the TRANSPOSED type matrix in LDS, edges on N) and dA_t += G^T X (both
// operands straight from the row-major edge tiles: one 4-byte LDS read per operand and k step, a 2x2 block of output
// tiles per wave), G = dm rows (or dagg rows at the edges' targets), X = h rows at their sources.  A workgroup walks a
// contiguous range of segments: the type's transposed matrix stays in LDS and its dA accumulators (16 registers per
// thread) in registers until the type changes, when they are added to dA with float atomics (dh likewise, as in the
// VALU kernel above: several edges share a source row).  Edge indices run three segments ahead of the MFMAs (sorted
// position -> edge slot -> its rows -> the two 512-byte rows), one stage per iteration, so that no request waits on a
// load issued in the same iteration; segments past the workgroup's range are clamped to its last one.
// The VALU kernel took 1.7 ms per call at 4096 molecules x D = 128 (1.3 % of the f32 MFMA peak for 10.7 GFLOP).
// ---------------------------------------------------------------------------------------
constexpr int kBwdMfmaMaxTypes = 1024;

template <int NT>
__global__ __launch_bounds__(1024) void bmm_message_typed_bwd_mfma_kernel(
    const float* __restrict__ h, const int32_t* __restrict__ conn, const float* __restrict__ A,
    const float* __restrict__ dm, float* __restrict__ dh, float* __restrict__ dA, const int32_t* __restrict__ start,
    const int32_t* __restrict__ segbase, const int32_t* __restrict__ order, int N, int E, int Vb, int from_agg,
    int owner_mode, float* __restrict__ du) {
  // du (optional, (B,E,D) with zero rows at masked edges): the per-edge vectors A_t^T g_e go to their edge slot's row with
  // plain 16-byte stores and a slot-order pass (reduce_scatter_kernel keyed by the source index) adds them into dh -
  // instead of float atomics on dh from here: 22 M of them at batch 4096 were 260 of the kernel's 349 us.
  // owner_mode (small batches): workgroup t takes ALL segments of bond type t and is the only one that touches dA_t,
  // which it updates with plain loads / adds / stores - flushing 64 KB of accumulators with float atomics after a
  // single segment costs ~50 us per workgroup (one 256-byte atomic wave-instruction per ~50 ns and CU).
  constexpr int D = 16 * NT, LD = D + 4, QD = D / 4, NLW = NT / 4, TI = NT / 4;
  constexpr int kX = kSeg * QD / 1024;  // 16-byte pieces of an edge tile per thread
  constexpr int kB = D * QD / 1024;     // ... of the matrix
  static_assert(kX >= 1 && kB >= 1 && NLW >= 1, "tile shape");
  extern __shared__ __align__(16) float smem[];
  float* AmT = smem;                // D x LD : AmT[j][i] = A_t[i][j]
  float* G = AmT + D * LD;          // kSeg x LD
  float* X = G + kSeg * LD;         // kSeg x LD
  int32_t* hrow_s = reinterpret_cast<int32_t*>(X + kSeg * LD);  // kSeg source rows (b * N + src)
  int32_t* sb_s = hrow_s + kSeg;    // segbase[0 .. Vb]
  int32_t* st_s = sb_s + Vb + 1;    // start[0 .. Vb]
  int32_t* be_s = st_s + Vb + 1;    // kSeg edge slots (b * E + e; -1 past the segment's edges) - with du
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  const int nseg = segbase[Vb];
  const int per = (nseg + (int)gridDim.x - 1) / (int)gridDim.x;
  int s0 = blockIdx.x * per, s1 = s0 + per < nseg ? s0 + per : nseg;
  if (owner_mode) {
    if ((int)blockIdx.x >= Vb) return;
    s0 = segbase[blockIdx.x];
    s1 = segbase[blockIdx.x + 1];
  }
  if (s0 >= s1) return;
  for (int t = tid; t <= Vb; t += 1024) {
    sb_s[t] = segbase[t];
    st_s[t] = start[t];
  }
  __syncthreads();
  struct Seg {
    int ty, p0, n;
  };
  auto seg_of = [&](int seg, int ty) {  // ty: a type at or before the segment's
    while (sb_s[ty + 1] <= seg) ++ty;
    Seg d;
    d.ty = ty;
    d.p0 = st_s[ty] + (seg - sb_s[ty]) * kSeg;
    d.n = min(kSeg, st_s[ty + 1] - d.p0);
    return d;
  };
  int ty0;
  {
    int lo = 0, hi = Vb - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sb_s[mid] <= s0) lo = mid; else hi = mid - 1;
    }
    ty0 = lo;
  }
  // pipeline stages, per thread and piece i < kX (edge e_i = (tid + 1024 i) / QD of the segment):
  //   stage C (3 ahead): be  = order[p0 + min(e, n - 1)]
  //   stage B (2 ahead): src, tgt = conn[be]                      -> rows
  //   stage A (1 ahead): the two 16-byte pieces of dm / h          -> registers -> LDS after the MFMAs
  int be_c[kX], be_b[kX], ok_b[kX];
  int hrow_a[kX], grow_a[kX], ok_a[kX];
  int64_t hrow_x[kX];
  f32x4_t gr[kX], xr[kX];
  int hrow_n[kX], ok_n[kX];  // of the pieces held in gr / xr
  int bes_a[kX], bes_n[kX];  // their edge slots (with du)
  auto stage_c = [&](const Seg& d, int* be, int* ok) {
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      const int e = (tid + 1024 * i) / QD;
      ok[i] = e < d.n;
      // (slots past the segment's edges borrow the rows of its real edges in turn: their zero sums are then spread
      //  over the segment's source rows - all of them on the LAST edge's row made 46 of 64 slots contend for one
      //  row at the reference's batch of 32: 99 vs 15 us per call)
      be[i] = order[d.p0 + (e < d.n ? e : e % d.n)];
    }
  };
  auto stage_b = [&](const int* be, int* hrow, int* grow, int* bes) {
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      const int b = be[i] / E;
      const int2 st = *reinterpret_cast<const int2*>(conn + (int64_t)be[i] * 2);
      hrow[i] = b * N + st.x;
      grow[i] = from_agg ? b * N + st.y : be[i];
      bes[i] = be[i];
    }
  };
  auto stage_a = [&](const int* hrow, const int* grow) {
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      const int c4 = (tid + 1024 * i) % QD;
      gr[i] = ldv4(dm + (int64_t)grow[i] * D + 4 * c4);
      xr[i] = ldv4(h + (int64_t)hrow[i] * D + 4 * c4);
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      const int idx = tid + 1024 * i, e = idx / QD, c4 = idx - e * QD;
      const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
      stv4(G + e * LD + 4 * c4, ok_n[i] ? gr[i] : zero);  // rows past the segment's edges are zero: they add nothing to dA
      stv4(X + e * LD + 4 * c4, ok_n[i] ? xr[i] : zero);
      if (c4 == 0) {
        hrow_s[e] = hrow_n[i];
        be_s[e] = ok_n[i] ? bes_n[i] : -1;
      }
    }
  };
  auto load_matrix = [&](int ty) {  // transposing copy: lanes run along i (conflict-free LDS stores)
#ifdef IMPNN_DIAG_BWD_NOMATRIX
    return;
#endif
    const float* At = A + (int64_t)ty * D * D;
#pragma unroll
    for (int i2 = 0; i2 < kB; ++i2) {
      const int idx = tid + 1024 * i2, i = idx % D, c4 = idx / D;
      const f32x4_t v = ldv4(At + (int64_t)i * D + 4 * c4);
#pragma unroll
      for (int r = 0; r < 4; ++r) AmT[(4 * c4 + r) * LD + i] = v[r];
    }
  };
  const int last = s1 - 1;
  Seg d0 = seg_of(s0, ty0);
  Seg d1 = seg_of(min(s0 + 1, last), d0.ty), d2 = seg_of(min(s0 + 2, last), d1.ty), d3 = seg_of(min(s0 + 3, last), d2.ty);
  // prologue: bring segment s0 into LDS, s0 + 1 to stage A, s0 + 2 to stage B, s0 + 3 to stage C
  {
    int be0[kX], ok0[kX], hr0[kX], gr0[kX];
    stage_c(d0, be0, ok0);
    stage_b(be0, hr0, gr0, bes_n);
    stage_a(hr0, gr0);
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      hrow_n[i] = hr0[i];
      ok_n[i] = ok0[i];
    }
    load_matrix(d0.ty);
    park();
    stage_c(d1, be0, ok0);
    stage_b(be0, hrow_a, grow_a, bes_a);
#pragma unroll
    for (int i = 0; i < kX; ++i) ok_a[i] = ok0[i];
    stage_c(d2, be_b, ok_b);
    stage_c(d3, be_c, ok_n);  // (ok of stage C travels with it below)
  }
  int ok_c[kX];
#pragma unroll
  for (int i = 0; i < kX; ++i) ok_c[i] = ok_n[i];
#pragma unroll
  for (int i = 0; i < kX; ++i) ok_n[i] = 1;  // placeholder until the first stage-A request below
  __syncthreads();
  const int et = wave & 3, fg = wave >> 2;          // GEMM 1: edge tile, feature group
  const int wi = wave & 3, wj = wave >> 2;          // GEMM 2: block of i tiles, block of j tiles
  f32x4_t acc2[TI][TI];
#pragma unroll
  for (int x = 0; x < TI; ++x)
#pragma unroll
    for (int y = 0; y < TI; ++y) acc2[x][y] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto flush_dA = [&](int ty) {
#ifdef IMPNN_DIAG_BWD_NOFLUSH
    return;
#endif
    float* dst = dA + (int64_t)ty * D * D;
#pragma unroll
    for (int x = 0; x < TI; ++x)
#pragma unroll
      for (int y = 0; y < TI; ++y) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float* pd = dst + (16 * (wi * TI + x) + 4 * q + g) * D + 16 * (wj * TI + y) + a;
          if (owner_mode) *pd += acc2[x][y][g];
          else atomicAdd(pd, acc2[x][y][g]);
        }
        acc2[x][y] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
  };
  for (int seg = s0; seg < s1; ++seg) {
    // requests for the segments ahead (each consumes what the previous iteration requested)
    int hrow_t[kX], ok_t[kX], bes_t[kX];
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      hrow_t[i] = hrow_a[i];
      ok_t[i] = ok_a[i];
      bes_t[i] = bes_a[i];
    }
    stage_a(hrow_a, grow_a);                 // rows of seg + 1
    stage_b(be_b, hrow_a, grow_a, bes_a);    // row indices of seg + 2
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      ok_a[i] = ok_b[i];
      be_b[i] = be_c[i];
      ok_b[i] = ok_c[i];
    }
    const Seg d4 = seg_of(min(seg + 4, last), d3.ty);
    stage_c(d4, be_c, ok_c);                 // edge slots of seg + 4
    __builtin_amdgcn_sched_barrier(0);
    // ---- GEMM 1: dh rows of this segment's edges
    {
      f32x4_t acc1[NLW];
#pragma unroll
      for (int TL = 0; TL < NLW; ++TL) acc1[TL] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const float* grow_p = G + (16 * et + a) * LD + 4 * q;
      const float* arow_p = AmT + (16 * (fg * NLW) + a) * LD + 4 * q;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const f32x4_t gv = ldv4(grow_p + 16 * u);
        f32x4_t av[NLW];
#pragma unroll
        for (int TL = 0; TL < NLW; ++TL) av[TL] = ldv4(arow_p + 16 * TL * LD + 16 * u);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int TL = 0; TL < NLW; ++TL) acc1[TL] = mfma_f32(av[TL][r], gv[r], acc1[TL]);
      }
      // (unconditional: rows past the segment's edges are zero in G, so their sums are exact zeros added to rows of
      //  the segment's real edges - a conditional atomic would keep the compiler from counting outstanding
      //  memory operations, and the LDS stores below would wait for every atomic of the tile)
#ifndef IMPNN_DIAG_BWD_NODH
      if (du) {  // (workgroup-uniform)
        const int bes = be_s[16 * et + a];
        if (bes >= 0) {
          float* dst = du + (int64_t)bes * D + 16 * (fg * NLW) + 4 * q;
#pragma unroll
          for (int TL = 0; TL < NLW; ++TL) stv4(dst + 16 * TL, acc1[TL]);
        }
      } else {
        float* dst = dh + (int64_t)hrow_s[16 * et + a] * D + 16 * (fg * NLW) + 4 * q;
#pragma unroll
        for (int TL = 0; TL < NLW; ++TL)
#pragma unroll
          for (int g = 0; g < 4; ++g) atomicAdd(dst + 16 * TL + g, acc1[TL][g]);
      }
#endif
    }
    // ---- GEMM 2: dA_t += G^T X over the segment's edges (k = edge)
#pragma unroll 4
    for (int sx = 0; sx < kSeg / 4; ++sx) {
      float gi[TI], xj[TI];
#pragma unroll
      for (int x = 0; x < TI; ++x) gi[x] = G[(4 * sx + q) * LD + 16 * (wi * TI + x) + a];
#pragma unroll
      for (int y = 0; y < TI; ++y) xj[y] = X[(4 * sx + q) * LD + 16 * (wj * TI + y) + a];
#pragma unroll
      for (int x = 0; x < TI; ++x)
#pragma unroll
        for (int y = 0; y < TI; ++y) acc2[x][y] = mfma_f32(gi[x], xj[y], acc2[x][y]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (seg + 1 >= s1) break;
    const bool new_type = d1.ty != d0.ty;  // (workgroup-uniform)
    if (new_type) flush_dA(d0.ty);
    __syncthreads();                       // every wave is done with G, X, hrow_s (and AmT)
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      hrow_n[i] = hrow_t[i];
      ok_n[i] = ok_t[i];
      bes_n[i] = bes_t[i];
    }
    park();
    if (new_type) load_matrix(d1.ty);
    __syncthreads();
    d0 = d1;
    d1 = d2;
    d2 = d3;
    d3 = d4;
  }
  flush_dA(d0.ty);
}

// ---------------------------------------------------------------------------------------
// a4 forward over the same type-sorted segments, for any D <= 128 (the D = 32 MFMA kernel of layer_kernels.hip
// keeps its own in-workgroup sort): A[type] sits in LDS with row stride D+1, so the lanes (output feature i) read
// their rows without bank conflicts - the per-molecule kernel reads A[type][i][:] with a stride of D floats between
// lanes, 64 cache lines per load.  Thread (edge lane, i) computes 4 edges at a time from one pass over its row.
// Masked / out-of-range edges get zero rows from a separate pass (models/layers.py:114-115).
// ---------------------------------------------------------------------------------------
__global__ void zero_invalid_messages_kernel(const int32_t* __restrict__ conn, const int32_t* __restrict__ bond_ids,
                                             float* __restrict__ m, int64_t BE, int N, int D, int Vb) {
  const int64_t total = BE * D;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t be = t / D;
    if (edge_type_or_neg(conn, bond_ids, be, N, Vb) < 0) m[t] = 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void bmm_message_typed_seg_kernel(
    const float* __restrict__ h, const int32_t* __restrict__ conn, const float* __restrict__ A,
    float* __restrict__ m_out, const int32_t* __restrict__ start, const int32_t* __restrict__ segbase,
    const int32_t* __restrict__ order, int N, int E, int D, int Vb) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int64_t outrow[kSeg];
  const int seg = blockIdx.x;
  if (seg >= segbase[Vb]) return;
  int lo = 0, hi = Vb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segbase[mid] <= seg) lo = mid; else hi = mid - 1;
  }
  const int ty = lo;
  const int p0 = start[ty] + (seg - segbase[ty]) * kSeg;
  const int n = min(kSeg, start[ty + 1] - p0);
  if (n <= 0) return;
  const int tid = threadIdx.x;
  const int LD = D + 1;
  float* As = smem;              // D x (D+1)
  float* xm = As + D * LD;       // kSeg x D, rows beyond n are zero
  for (int t = tid; t < D * D; t += kBlock) As[(t / D) * LD + (t % D)] = A[(int64_t)ty * D * D + t];
  for (int t = tid; t < kSeg * D; t += kBlock) {
    const int e = t / D, c = t - e * D;
    float v = 0.f;
    if (e < n) {
      const int64_t be = order[p0 + e];
      v = h[((be / E) * N + conn[be * 2]) * D + c];
      if (c == 0) outrow[e] = be;
    }
    xm[t] = v;
  }
  __syncthreads();
  const int lanes = kBlock / D > 0 ? kBlock / D : 1;
  if (tid < lanes * D) {
    const int i = tid % D, el = tid / D;
    const float* arow = As + i * LD;
    for (int e0 = 4 * el; e0 < n; e0 += 4 * lanes) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      const float* x = xm + e0 * D;
      for (int j = 0; j < D; ++j) {
        const float w = arow[j];
        a0 = fmaf(w, x[j], a0);
        a1 = fmaf(w, x[D + j], a1);
        a2 = fmaf(w, x[2 * D + j], a2);
        a3 = fmaf(w, x[3 * D + j], a3);
      }
      m_out[outrow[e0] * D + i] = a0;
      if (e0 + 1 < n) m_out[outrow[e0 + 1] * D + i] = a1;
      if (e0 + 2 < n) m_out[outrow[e0 + 2] * D + i] = a2;
      if (e0 + 3 < n) m_out[outrow[e0 + 3] * D + i] = a3;
    }
  }
}

// The same on the matrix cores for D a multiple of 16 (exact f32 products): per segment the GEMM
// m^T (D x 64) = A[type] (D x D) * x^T (D x 64) in 16x16 output tiles, K index ordered as 16u + 4q + r so that one
// 16-byte LDS read per lane feeds four MFMA steps of both operands.  Wave w owns the output tiles w, w+4, ...
__global__ __launch_bounds__(1024) void bmm_message_typed_seg_mfma_kernel(
    const float* __restrict__ h, const int32_t* __restrict__ conn, const float* __restrict__ A,
    float* __restrict__ m_out, const int32_t* __restrict__ start, const int32_t* __restrict__ segbase,
    const int32_t* __restrict__ order, int N, int E, int D, int Vb, int segs_per_wg) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int64_t outrow[kSeg];
  const int nseg = segbase[Vb];
  const int tid = threadIdx.x;
  const int LD = D + 4;            // 16-byte aligned rows, bank-staggered
  float* As = smem;                // D x LD
  float* xm = As + D * LD;         // kSeg x LD, rows beyond n are zero
  const int D4 = D >> 2;
  const int lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  // A workgroup walks `segs_per_wg` consecutive segments: segments of one type are numbered consecutively, so the
  // type's matrix (D*D*4 bytes - 64 KB at D = 128: the segment's dominant cost, not its MFMAs) stays in LDS until the
  // type changes instead of being copied once per 64 edges.
  int held = -1;
  for (int seg = blockIdx.x * segs_per_wg; seg < (blockIdx.x + 1) * segs_per_wg && seg < nseg; ++seg) {
    int lo = 0, hi = Vb - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segbase[mid] <= seg) lo = mid; else hi = mid - 1;
    }
    const int ty = lo;
    const int p0 = start[ty] + (seg - segbase[ty]) * kSeg;
    const int n = min(kSeg, start[ty + 1] - p0);
    if (n <= 0) continue;  // (workgroup-uniform)
    __syncthreads();       // the previous segment's MFMAs are done with xm / outrow (and As, if the type changes)
    // 16-byte loads throughout (D is a multiple of 16, rows of A / h / the LDS tiles are 16-byte aligned)
    if (ty != held) {
      held = ty;
      const float* Aty = A + (int64_t)ty * D * D;
      for (int t = tid; t < D * D4; t += (int)blockDim.x) {
        const int r = t / D4, c4 = t - r * D4;
        stv4(As + r * LD + 4 * c4, ldv4(Aty + (int64_t)r * D + 4 * c4));
      }
    }
    if (tid < kSeg) outrow[tid] = tid < n ? (int64_t)order[p0 + tid] : 0;
    __syncthreads();
    for (int t = tid; t < kSeg * D4; t += (int)blockDim.x) {
      const int e = t / D4, c4 = t - e * D4;
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (e < n) {
        const int64_t be = outrow[e];
        v = ldv4(h + ((be / E) * N + conn[be * 2]) * D + 4 * c4);
      }
      stv4(xm + e * LD + 4 * c4, v);
    }
    __syncthreads();
    const int mt = D >> 4, et = (n + 15) >> 4;          // output tiles: features x edges
    for (int tile = wave; tile < mt * et; tile += (int)blockDim.x >> 6) {
      const int T = tile % mt, Et = tile / mt;
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      const float* arow = As + (16 * T + a) * LD + 4 * q;
      const float* xrow = xm + (16 * Et + a) * LD + 4 * q;
      for (int u = 0; u < mt; ++u) {
        const f32x4_t av = ldv4(arow + 16 * u), xv = ldv4(xrow + 16 * u);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma_f32(av[r], xv[r], acc);
      }
      const int e = 16 * Et + a;                        // accumulator: feature 16T + 4q + reg of edge e
      if (e < n) stv4(m_out + outrow[e] * D + 16 * T + 4 * q, acc);
    }
  }
}

}  // namespace

int64_t bmm_message_typed_bwd_workspace_ints(int B, int E, int Vb) { return (int64_t)4 * (Vb + 1) + (int64_t)B * E; }

// the batch's valid edges, counting-sorted by bond type, into the call's workspace
static int launch_edge_type_sort(const TypedMessageCall& c, const EdgeSortView& v) {
  const int64_t BE = (int64_t)c.B * c.E;
  if (BE <= 1024 * kSortSmallPer && c.Vb <= 1024) {
    edge_type_sort_small_kernel<<<1, 1024, 0, c.stream>>>(c.conn, c.bond_ids, v.cnt, v.start, v.cursor, v.segbase,
                                                          v.order, (int)BE, c.N, c.Vb);
    return check_launch("edge_type_sort_small");
  }
  // (a kernel, not hipMemsetAsync: the call must behave the same inside a captured hipGraph)
  zero_ints_kernel<<<grid_for(c.Vb + 1), kBlock, 0, c.stream>>>(v.cnt, c.Vb + 1);
  if (int rc = check_launch("zero_ints")) return rc;
  const int sort_grid = grid_for(BE / 8 + 1, 512);
  edge_type_hist_kernel<<<sort_grid, kBlock, 0, c.stream>>>(c.conn, c.bond_ids, v.cnt, BE, c.N, c.Vb);
  if (int rc = check_launch("edge_type_hist")) return rc;
  edge_type_prefix_kernel<<<1, 64, 0, c.stream>>>(v.cnt, v.start, v.cursor, v.segbase, c.Vb);
  if (int rc = check_launch("edge_type_prefix")) return rc;
  edge_type_scatter_kernel<<<sort_grid, kBlock, 0, c.stream>>>(c.conn, c.bond_ids, v.cursor, v.order, BE, c.N, c.Vb);
  return check_launch("edge_type_scatter");
}

int launch_bmm_message_typed_sorted(const TypedMessageCall& c) {
  const EdgeSortView v(c.workspace, c.Vb);
  const int D = c.D;
  const int64_t BE = (int64_t)c.B * c.E;
  hipStream_t s = c.stream;
  if (!c.sort_ready)
    if (int rc = launch_edge_type_sort(c, v)) return rc;
  if (!c.zero_rows_ready) {  // (else: the caller's buffer still holds the zero rows of an earlier call on this batch)
    zero_invalid_messages_kernel<<<grid_for(BE * D), kBlock, 0, s>>>(c.conn, c.bond_ids, c.messages, BE, c.N, D, c.Vb);
    if (int rc = check_launch("zero_invalid_messages")) return rc;
  }
  const int64_t max_segs = (BE + kSeg - 1) / kSeg + c.Vb;
  if (D % 16 == 0 && aligned16(c.messages) && aligned16(c.type_mats) && aligned16(c.h)) {
    const size_t lm = sizeof(float) * ((size_t)D * (D + 4) + (size_t)kSeg * (D + 4));
    if (lm > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)bmm_message_typed_seg_mfma_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lm);
    // wide states: 16 waves (4 per SIMD) share the segment's 32 output tiles, so LDS reads overlap the MFMAs
    // wide states: several segments per workgroup (the matrix copy is amortised); keep >= ~4 workgroups per CU of work
    int spw = D >= 64 ? (int)(max_segs / 1024) : 1;
    spw = spw < 1 ? 1 : (spw > 8 ? 8 : spw);
    bmm_message_typed_seg_mfma_kernel<<<(int)((max_segs + spw - 1) / spw), D >= 64 ? 1024 : kBlock, lm, s>>>(
        c.h, c.conn, c.type_mats, c.messages, v.start, v.segbase, v.order, c.N, c.E, D, c.Vb, spw);
    return check_launch("bmm_message_typed_seg_mfma");
  }
  const size_t lds = sizeof(float) * ((size_t)D * (D + 1) + (size_t)kSeg * D);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)bmm_message_typed_seg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  bmm_message_typed_seg_kernel<<<(int)max_segs, kBlock, lds, s>>>(c.h, c.conn, c.type_mats, c.messages, v.start,
                                                                  v.segbase, v.order, c.N, c.E, D, c.Vb);
  return check_launch("bmm_message_typed_seg");
}

template <int NT>
static int launch_bwd_mfma(const TypedMessageCall& c, const EdgeSortView& v, int grid, size_t lds, int owner) {
  (void)hipFuncSetAttribute((const void*)bmm_message_typed_bwd_mfma_kernel<NT>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  bmm_message_typed_bwd_mfma_kernel<NT><<<grid, 1024, lds, c.stream>>>(
      c.h, c.conn, c.type_mats, c.grad, c.dh, c.dtype_mats, v.start, v.segbase, v.order, c.N, c.E, c.Vb, c.from_agg,
      owner, c.edge_scratch);
  return check_launch("bmm_message_typed_bwd (mfma)");
}

template <int ACC>
static int launch_bwd_valu(const TypedMessageCall& c, const EdgeSortView& v, int grid, int threads, size_t lds) {
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)bmm_message_typed_bwd_kernel<ACC>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  bmm_message_typed_bwd_kernel<ACC><<<grid, threads, lds, c.stream>>>(
      c.h, c.conn, c.type_mats, c.grad, c.dh, c.dtype_mats, v.start, v.segbase, v.order, c.N, c.E, c.D, c.Vb,
      c.from_agg, c.edge_scratch);
  return check_launch("bmm_message_typed_bwd");
}

int launch_bmm_message_typed_bwd(const TypedMessageCall& c) {
  const EdgeSortView v(c.workspace, c.Vb);
  const int D = c.D;
  // IMPNN_MESSAGE_BWD (diagnostics: "valu" / "mfma" / "mo"): read on every call, as tests switch it inside one process
  const char* force = getenv("IMPNN_MESSAGE_BWD");
  const bool mfma = (D == 64 || D == 128) && c.Vb <= kBwdMfmaMaxTypes && (!force || force[0] == 'm') &&
                    aligned16(c.h) && aligned16(c.type_mats) && aligned16(c.grad) &&
                    (reinterpret_cast<uintptr_t>(c.conn) & 7u) == 0;
  // the matrix-core kernel writes the per-edge vectors with 16-byte stores (refused before anything is launched)
  if (mfma && c.edge_scratch && !aligned16(c.edge_scratch))
    return fail(IMPNN_E_BADARG, "%s: the per-edge buffer must be 16B aligned", c.entry);
  if (!c.sort_ready)  // the sort depends on (conn, bond_ids) only: forward and backward of the S layers of an ion share it
    if (int rc = launch_edge_type_sort(c, v)) return rc;
  const int64_t max_segs = ((int64_t)c.B * c.E + kSeg - 1) / kSeg + c.Vb;
  int rc;
  if (mfma) {
    const size_t lm = sizeof(float) * ((size_t)D * (D + 4) + 2 * (size_t)kSeg * (D + 4)) +
                      sizeof(int32_t) * (2 * kSeg + 2 * (size_t)(c.Vb + 1));
    // one workgroup per type without atomics on dA ("mo", diagnostics) was never faster than balanced segment ranges:
    // 26.8 vs 26.1 us per call at batch 32, 423 vs 331 us at batch 4096 (VALU kernel: 41.7 / 887 us)
    const int owner = force && force[1] == 'o' ? 1 : 0;
    const int grid = owner ? c.Vb : (int)(max_segs < 256 ? max_segs : 256);
    rc = D == 128 ? launch_bwd_mfma<8>(c, v, grid, lm, owner) : launch_bwd_mfma<4>(c, v, grid, lm, owner);
  } else {
    const size_t lds = sizeof(float) * ((size_t)D * D + 2 * (size_t)kSeg * D);
    // wide states need > 64 KB of LDS (one workgroup per CU): 16 waves instead of 4 keep every SIMD busy
    const int threads = D >= 64 ? 1024 : kBlock;
    const int acc = (D * D + threads - 1) / threads;  // accumulators per thread: <= 16, as D <= 128
    rc = acc <= 1   ? launch_bwd_valu<1>(c, v, (int)max_segs, threads, lds)
         : acc <= 4 ? launch_bwd_valu<4>(c, v, (int)max_segs, threads, lds)
                    : launch_bwd_valu<16>(c, v, (int)max_segs, threads, lds);
  }
  if (rc || !c.edge_scratch) return rc;
  // the per-edge vectors, added into dh at their source rows in edge-slot order (conn[b, e, 0]: stride 2)
  return launch_reduce_scatter_add(c.edge_scratch, c.conn, 2, c.dh, c.B, c.N, c.E, D, c.stream, 1);
}

}  // namespace impnn
