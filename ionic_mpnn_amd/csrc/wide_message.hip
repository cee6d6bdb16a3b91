// The message stage of the wide encoder (encoder_wide.hip has the stage list): wide_message (exact f32),
// wide_message_x3 (mode f32x3, bf16x9) and wide_reduce.
#include "wide_device.h"

namespace impnn {
namespace wide {

// a4 over the type-sorted edge list.  A workgroup walks a contiguous range of TE-edge tiles; tiles of one type are
// consecutive, so the type's D x D matrix (64 KB at D = 128) stays in LDS until the type changes.  Output tile =
// (features on M) x (edges on N): lane (a, q) of the accumulator of feature tile T holds features 16T + 4q .. +3 of
// edge a - one 16-byte store per tile.  The next tile's source rows (and, at a type change, the next matrix) are
// requested before the MFMAs of the current tile and stored to the other LDS buffer after them.
template <int NT, int TE>
__global__ __launch_bounds__(1024) void wide_message_kernel(MsgParams p) {
  constexpr int D = 16 * NT, LD = D + 4, QD = D / 4;
  constexpr int EG = TE / 16, FG = 16 / EG, NLW = NT / FG;  // edge tiles, feature groups, feature tiles per wave
  constexpr int kX = TE * QD / 1024, kB = D * QD / 1024;    // 16-byte pieces per thread: a tile of rows, the matrix
  static_assert(kX >= 1 && kB >= 1 && NLW >= 1, "tile shape");
  extern __shared__ __align__(16) float smem[];
  float* Bm = smem;               // D x LD
  float* Xb = Bm + D * LD;        // 2 x TE x LD
  int32_t* tb_s = reinterpret_cast<int32_t*>(Xb + 2 * TE * LD);  // tilebase[0 .. nT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  const int et = wave % EG, fg = wave / EG;
  const int ntiles = p.meta[kMetaTiles];
  const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  if (t0 >= t1) return;
  WIDE_STAMP(p.stamps, 0);
  WIDE_STAMP_REAL(p.stamps, 5);
  for (int t = tid; t <= p.nT; t += 1024) tb_s[t] = p.tilebase[t];
  __syncthreads();
  auto mat_of = [&](int t) {
    const int g = t >= p.Vb ? 1 : 0;
    return p.img[g] + p.mat_off + (size_t)(t - g * p.Vb) * D * D;
  };
  // A type's run starts at a multiple of TE sorted positions (wide_scan), so tile t is positions [t TE, (t + 1) TE):
  // positions past the type's last edge are padding - their source row is row 0 (wide_scan), their messages are
  // computed and stored like any other and never read.  No load or store of the loop is conditional, which lets the
  // compiler count outstanding memory operations instead of draining them: source rows are requested TWO tiles ahead
  // (sr2), the rows themselves one tile ahead (xr), the stores of a tile drain under the next tile's MFMAs.
  int sr1[kX], sr2[kX];
  f32x4_t xr[kX], br[kB];
  auto fetch_sr = [&](int tile, int* sr) {
#pragma unroll
    for (int i = 0; i < kX; ++i) sr[i] = p.srcrow[tile * TE + (tid + 1024 * i) / QD];
  };
  auto fetch_x = [&](const int* sr) {
#pragma unroll
    for (int i = 0; i < kX; ++i) xr[i] = ldv4(p.h + (int64_t)sr[i] * D + 4 * ((tid + 1024 * i) % QD));
  };
  auto park_x = [&](float* X) {
#pragma unroll
    for (int i = 0; i < kX; ++i) {
      const int idx = tid + 1024 * i, e = idx / QD, c4 = idx - e * QD;
      stv4(X + e * LD + 4 * c4, xr[i]);
    }
  };
  auto fetch_b = [&](int t) {
    const float* A = mat_of(t);
#pragma unroll
    for (int i = 0; i < kB; ++i) br[i] = ldv4(A + (size_t)(tid + 1024 * i) * 4);
  };
  auto park_b = [&]() {
#pragma unroll
    for (int i = 0; i < kB; ++i) {
      const int idx = tid + 1024 * i, r = idx / QD, c4 = idx - r * QD;
      stv4(Bm + r * LD + 4 * c4, br[i]);
    }
  };
  int ty;
  {  // type of the first tile: largest t with tilebase[t] <= t0 (empty types share a base with their successor)
    int lo = 0, hi = p.nT - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tb_s[mid] <= t0) lo = mid; else hi = mid - 1;
    }
    ty = lo;
  }
  int run_end = tb_s[ty + 1];  // first tile of the next type
  fetch_sr(t0, sr1);
  fetch_b(ty);
  fetch_x(sr1);
  fetch_sr(min(t0 + 1, t1 - 1), sr1);
  park_x(Xb);
  park_b();
  __syncthreads();
  WIDE_STAMP(p.stamps, 1);
  int cur = 0;
  for (int tile = t0; tile < t1; ++tile) {
    // the next tile (the last tile is simply requested again: no branch around the requests)
    const int nxt = min(tile + 1, t1 - 1);
    int ty2 = ty, run_end2 = run_end;
    if (nxt >= run_end) {  // (workgroup-uniform) a new type: step over empty ones
      do {
        ++ty2;
        run_end2 = tb_s[ty2 + 1];
      } while (run_end2 <= nxt);
      fetch_b(ty2);
    }
    fetch_x(sr1);
    fetch_sr(min(tile + 2, t1 - 1), sr2);
    __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks the requests below the MFMAs, next to their use)
    {
      const float* X = Xb + cur * TE * LD;
      f32x4_t acc[NLW];
#pragma unroll
      for (int TL = 0; TL < NLW; ++TL) acc[TL] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const float* xrow = X + (16 * et + a) * LD + 4 * q;
      const float* arow = Bm + (16 * (fg * NLW) + a) * LD + 4 * q;
#pragma unroll
      for (int u = 0; u < NT; ++u) {
#ifdef IMPNN_DIAG_WIDE_NOLDS
        const f32x4_t xv = {1.f + u, 2.f, 3.f, 4.f};
        f32x4_t av[NLW];
#pragma unroll
        for (int TL = 0; TL < NLW; ++TL) av[TL] = f32x4_t{0.5f, 0.25f + TL, 0.125f, 2.f};
#else
        const f32x4_t xv = ldv4(xrow + 16 * u);
        f32x4_t av[NLW];
#pragma unroll
        for (int TL = 0; TL < NLW; ++TL) av[TL] = ldv4(arow + 16 * TL * LD + 16 * u);
#endif
#ifdef IMPNN_DIAG_WIDE_NOMMA
        acc[0] += xv + av[0] + av[NLW - 1];
#else
#pragma unroll
        for (int TL = 0; TL < NLW; ++TL)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[TL] = mfma_f32(av[TL][r], xv[r], acc[TL]);
#endif
      }
      float* dst = p.m + ((int64_t)tile * TE + 16 * et + a) * D + 16 * (fg * NLW) + 4 * q;
#pragma unroll
      for (int TL = 0; TL < NLW; ++TL) stv4(dst + 16 * TL, acc[TL]);
    }
    __builtin_amdgcn_sched_barrier(0);
    park_x(Xb + (cur ^ 1) * TE * LD);
    if (ty2 != ty) {     // (workgroup-uniform)
      __syncthreads();   // every wave is done with the old matrix
      park_b();
    }
    __syncthreads();
    cur ^= 1;
    ty = ty2;
    run_end = run_end2;
#pragma unroll
    for (int i = 0; i < kX; ++i) sr1[i] = sr2[i];
  }
  WIDE_STAMP(p.stamps, 4);
  WIDE_STAMP_REAL(p.stamps, 6);
#ifdef IMPNN_DIAG_WIDE_STAMPS
  if (p.stamps && threadIdx.x == 0) p.stamps[(size_t)blockIdx.x * 8 + 7] = (unsigned long long)(t1 - t0);
#endif
}

// ------------------------------------------------------------------------------------------------------------
// a2 + a4 in mode IMPNN_ENCODER_F32X3_TYPED: the per-type GEMMs m = A[type] h[src] on the bf16 matrix pipe, every f32
// operand carried exactly as three bf16 terms and all nine cross products accumulated in f32 (as the GatedUpdate of this
// mode).  8 waves: a wave multiplies 32 edges x 32 features (2 x 2 MFMA tiles; 64-edge tiles at D = 128, 128-edge tiles
// at D = 64 - as the plan cuts them).
//   * a wave keeps ITS operands of the type's matrix - 32 feature rows, all k, three planes: 96 VGPRs - in registers
//     for the whole run of the type (a type's run is ~40 tiles; the planes come pre-split and in operand order from
//     the prepared image, wide_mat_planes_kernel), so a tile costs LDS traffic for the rows only;
//   * the rows of the next tile are gathered under the MFMAs, split (three planes of bf16) and parked in the other of
//     two LDS stages between the MFMAs of the second half of the tile: one barrier per tile.
// Tiles, runs and the unconditional requests as in wide_message_kernel.
// ------------------------------------------------------------------------------------------------------------
constexpr int kMsgX3Threads = 512;
constexpr size_t msg_x3_lds_bytes(int D, int TE, int nT) { return 2 * (size_t)3 * (D / 32) * 4 * (TE + 1) * 16 + (size_t)(nT + 1) * 4; }

template <int NT, int TE>
__global__ __launch_bounds__(kMsgX3Threads, 1) void wide_message_x3_kernel(MsgParams p) {
  constexpr int D = 16 * NT, QD = D / 4, KB = D / 32, T = kMsgX3Threads;
  constexpr int UM = 3 * KB * 4 * D;   // 16-byte units of a type's matrix (three planes): [plane][k block][k octet][feature]
  constexpr int XS = TE + 1;           // units between the (k block, k octet) rows of a tile's planes: one unit of padding, so
                                       // that the 16 k octets a wave parks at once fall into different LDS banks
  constexpr int UX = 3 * KB * 4 * XS;  // ... of a tile of rows: [plane][k block][k octet][edge]
  constexpr int kX = TE * QD / T;      // 16-byte pieces of f32 rows per thread
  constexpr int EGN = TE / 32, FGN = 8 / EGN;  // 8 waves = EGN groups of 32 edges x FGN groups of 32 features
  static_assert(EGN * FGN == 8 && NT == 2 * FGN && kX >= 2 && kX % 2 == 0 && KB % 2 == 0, "tile shape");
  extern __shared__ __align__(16) unsigned char smem_b[];
  uint4* const Xb = reinterpret_cast<uint4*>(smem_b);             // 2 x UX units
  int32_t* const tb_s = reinterpret_cast<int32_t*>(Xb + 2 * UX);  // tilebase[0 .. nT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 15, q = lane >> 4;
  const int eg = wave % EGN, fg = wave / EGN;  // 32 edges x 32 features
  const int ntiles = p.meta[kMetaTiles];
  const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int t0 = blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  if (t0 >= t1) return;
  WIDE_STAMP(p.stamps, 0);
  WIDE_STAMP_REAL(p.stamps, 5);
  bf16x8_t am[KB][2][3];  // the wave's matrix operands: [k block][feature tile][plane]
  auto load_mat = [&](int t) {
    const int g = t >= p.Vb ? 1 : 0;
    const uint4* src = reinterpret_cast<const uint4*>(p.img[g] + p.planes_off) + (size_t)(t - g * p.Vb) * UM;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int TL = 0; TL < 2; ++TL)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          am[kb][TL][pl] = __builtin_bit_cast(bf16x8_t, src[((pl * KB + kb) * 4 + q) * D + 16 * (fg * 2 + TL) + a]);
  };
  auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  // rows are requested TWO tiles ahead (two sets of staging registers, alternating), their source-row indices three
  int srn[kX];
  f32x4_t xa[kX], xb[kX];
  auto fetch_sr = [&](int tile) {
#pragma unroll
    for (int i = 0; i < kX; ++i) srn[i] = p.srcrow[tile * TE + (tid + T * i) / QD];
  };
  auto fetch_x = [&](f32x4_t (&xr)[kX]) {  // the rows srn names
#pragma unroll
    for (int i = 0; i < kX; ++i) xr[i] = ldv4(p.h + (int64_t)srn[i] * D + 4 * ((tid + T * i) % QD));
  };
  auto park_piece = [&](uint4* X, const f32x4_t (&xr)[kX], int i) {  // 4 values of a row -> three planes of 4 bf16:
    uint2* s2 = reinterpret_cast<uint2*>(X);                          // unit (plane, k block, k octet, edge), 8-byte half
    const int idx = tid + T * i, e = idx / QD, c4 = idx - e * QD;
    const int un = ((c4 >> 3) * 4 + ((c4 >> 1) & 3)) * XS + e, half = c4 & 1;
    unsigned w0[2], w1[2], w2[2];
    split_pair(xr[i][0], xr[i][1], w0[0], w1[0], w2[0]);
    split_pair(xr[i][2], xr[i][3], w0[1], w1[1], w2[1]);
    s2[(0 * KB * 4 * XS + un) * 2 + half] = make_uint2(w0[0], w0[1]);
    s2[(1 * KB * 4 * XS + un) * 2 + half] = make_uint2(w1[0], w1[1]);
    s2[(2 * KB * 4 * XS + un) * 2 + half] = make_uint2(w2[0], w2[1]);
  };
  // (the first source rows are requested together with the run table: one round trip to memory instead of two)
  const int tl = t1 - 1;  // (requests past the share's last tile name it again: no branch around them)
  fetch_sr(t0);
  for (int t = tid; t <= p.nT; t += T) tb_s[t] = p.tilebase[t];
  __syncthreads();
  int ty;
  {  // type of the first tile: largest t with tilebase[t] <= t0 (empty types share a base with their successor)
    int lo = 0, hi = p.nT - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tb_s[mid] <= t0) lo = mid; else hi = mid - 1;
    }
    ty = lo;
  }
  int run_end = tb_s[ty + 1];  // first tile of the next type
  fetch_x(xa);                    // rows of t0
  load_mat(ty);
  fetch_sr(min(t0 + 1, tl));
#pragma unroll
  for (int i = 0; i < kX; ++i) park_piece(Xb, xa, i);
  fetch_x(xa);                    // rows of t0 + 1: parked inside tile t0
  fetch_sr(min(t0 + 2, tl));      // (srn = the rows of t0 + 2: requested at the top of tile t0)
  lds_barrier();
  WIDE_STAMP(p.stamps, 1);
  constexpr int kPa[9] = {2, 1, 2, 0, 2, 1, 0, 1, 0}, kPb[9] = {2, 2, 1, 2, 0, 1, 1, 0, 0};  // (matrix plane, row plane), smallest first
  int cur = 0;
  // tile `tile` out of stage cur; the rows of tile + 1 (in xpark since the tile before) go to the other stage, the rows
  // of tile + 2 are requested into xfetch
  auto do_tile = [&](int tile, f32x4_t (&xpark)[kX], f32x4_t (&xfetch)[kX]) {
    const int nxt = min(tile + 1, tl);
    int ty2 = ty, run_end2 = run_end;
    if (nxt >= run_end) {  // (workgroup-uniform) a new type: step over empty ones
      do {
        ++ty2;
        run_end2 = tb_s[ty2 + 1];
      } while (run_end2 <= nxt);
    }
    fetch_x(xfetch);
    fetch_sr(min(tile + 3, tl));
    __builtin_amdgcn_sched_barrier(0);
    {
      const uint4* X = Xb + cur * UX;
      f32x4_t acc[2][2];  // [feature tile][edge tile]
#pragma unroll
      for (int TL = 0; TL < 2; ++TL)
#pragma unroll
        for (int et = 0; et < 2; ++et) acc[TL][et] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      bf16x8_t xe[2][2][3];  // [buffer][edge tile][plane]
#pragma unroll
      for (int pl = 2; pl >= 0; --pl)  // (in the order the products take them)
#pragma unroll
        for (int et = 0; et < 2; ++et)
          xe[0][et][pl] = __builtin_bit_cast(bf16x8_t, X[((pl * KB + 0) * 4 + q) * XS + 16 * (eg * 2 + et) + a]);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        if (kb + 1 < KB) {
#pragma unroll
          for (int pl = 2; pl >= 0; --pl)
#pragma unroll
            for (int et = 0; et < 2; ++et)
              xe[(kb + 1) & 1][et][pl] = __builtin_bit_cast(bf16x8_t, X[((pl * KB + kb + 1) * 4 + q) * XS + 16 * (eg * 2 + et) + a]);
        }
        // the next tile's rows (requested at the top of this one) are split and parked between the MFMAs of the last
        // two k blocks: half of the thread's pieces each
        if (kb >= KB - 2) {
#pragma unroll
          for (int i = (kb - (KB - 2)) * (kX / 2); i < (kb - (KB - 2) + 1) * (kX / 2); ++i) park_piece(Xb + (cur ^ 1) * UX, xpark, i);
        }
#pragma unroll
        for (int pr = 0; pr < 9; ++pr)
#pragma unroll
          for (int TL = 0; TL < 2; ++TL)
#pragma unroll
            for (int et = 0; et < 2; ++et)
              acc[TL][et] = mfma_bf16(am[kb][TL][kPa[pr]], xe[kb & 1][et][kPb[pr]], acc[TL][et]);
        if (kb >= KB - 2) {
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // VALU
          }
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS write
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int et = 0; et < 2; ++et) {
        float* dst = p.m + ((int64_t)tile * TE + 16 * (eg * 2 + et) + a) * D + 16 * (fg * 2) + 4 * q;
#pragma unroll
        for (int TL = 0; TL < 2; ++TL) stv4(dst + 16 * TL, acc[TL][et]);
      }
    }
    if (ty2 != ty) load_mat(ty2);  // (workgroup-uniform; its latency is exposed once per type run)
    lds_barrier();  // the other stage is complete, this one free: the stores above stay in flight
    cur ^= 1;
    ty = ty2;
    run_end = run_end2;
  };
  for (int tile = t0; tile < t1; tile += 2) {
    do_tile(tile, xa, xb);
    if (tile + 1 < t1) do_tile(tile + 1, xb, xa);
  }
  WIDE_STAMP(p.stamps, 4);
  WIDE_STAMP_REAL(p.stamps, 6);
#ifdef IMPNN_DIAG_WIDE_STAMPS
  if (p.stamps && threadIdx.x == 0) p.stamps[(size_t)blockIdx.x * 8 + 7] = (unsigned long long)(t1 - t0);
#endif
}

// a5 on the compact rows: D/4 lanes per row, the in-edge messages added in edge-slot order with 4 rows in flight.
__global__ __launch_bounds__(256) void wide_reduce_kernel(const float* __restrict__ m, const int2* __restrict__ rowinfo,
                                                          const int32_t* __restrict__ csr, float* __restrict__ agg,
                                                          const int32_t* __restrict__ meta, int n_ions, int D, int skip_upto) {
  const int qd = D >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / qd;
  const int c4 = (int)(t - row * qd);
  if (row >= meta[kMetaEnd]) return;
  if (n_ions > 1 && row >= meta[kMetaRows] && row < meta[kMetaBase + 1]) return;  // the gap in front of ion 1
  const int2 ri = rowinfo[row];
  if (ri.y <= skip_upto) return;  // the update adds up to two messages itself, and zeros for a row without in-edges (wide_iota_kernel)
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  int i = 0;
  for (; i + 4 <= ri.y; i += 4) {
    const int p0 = csr[ri.x + i], p1 = csr[ri.x + i + 1], p2 = csr[ri.x + i + 2], p3 = csr[ri.x + i + 3];
    const f32x4_t v0 = ldv4(m + (int64_t)p0 * D + 4 * c4), v1 = ldv4(m + (int64_t)p1 * D + 4 * c4);
    const f32x4_t v2 = ldv4(m + (int64_t)p2 * D + 4 * c4), v3 = ldv4(m + (int64_t)p3 * D + 4 * c4);
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; i < ri.y; ++i) acc += ldv4(m + (int64_t)csr[ri.x + i] * D + 4 * c4);
  stv4(agg + row * D + 4 * c4, acc);
}

// Persistent workgroups: one per CU.
int launch_wide_message(const MsgParams& p, int D, int te, bool x3_msg, int cus, hipStream_t s) {
  if (x3_msg) {
    const size_t lds = msg_x3_lds_bytes(D, te, p.nT);
    if (D == 128) {
      if (int rc = raise_lds<wide_message_x3_kernel<8, 64>>(lds)) return rc;
      wide_message_x3_kernel<8, 64><<<cus, kMsgX3Threads, lds, s>>>(p);
    } else {
      if (int rc = raise_lds<wide_message_x3_kernel<4, 128>>(lds)) return rc;
      wide_message_x3_kernel<4, 128><<<cus, kMsgX3Threads, lds, s>>>(p);
    }
    return IMPNN_OK;
  }
  const size_t lds = ((size_t)D * (D + 4) + 2 * (size_t)te * (D + 4)) * 4 + (size_t)(p.nT + 1) * 4;
  if (D == 128) {
    if (int rc = raise_lds<wide_message_kernel<8, 64>>(lds)) return rc;
    wide_message_kernel<8, 64><<<cus, 1024, lds, s>>>(p);
  } else {
    if (int rc = raise_lds<wide_message_kernel<4, 128>>(lds)) return rc;
    wide_message_kernel<4, 128><<<cus, 1024, lds, s>>>(p);
  }
  return IMPNN_OK;
}

void launch_wide_reduce(const Ws& w, void* workspace, int n_ions, int D, bool direct, hipStream_t s) {
  char* base = static_cast<char*>(workspace);
  const int64_t threads = w.rmax * (D / 4);
  wide_reduce_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(
      reinterpret_cast<const float*>(base + w.m), reinterpret_cast<const int2*>(base + w.rowinfo),
      reinterpret_cast<const int32_t*>(base + w.csr), reinterpret_cast<float*>(base + w.agg),
      reinterpret_cast<const int32_t*>(base + w.meta), n_ions, D, direct ? 2 : 0);
}

}  // namespace wide
}  // namespace impnn
