// encode() for wide atom states (atom_dim 64 / 128: BASELINE config 5, train_viscosity.py:166-190 with atom_dim=128,
// num_steps=6) behind the encoder entries of include/impnn.h, mode IMPNN_ENCODER_F32_TYPED.
//
// At D = 128 a row of node state is 512 bytes and a GatedUpdate weight set 394 KB: nothing of the D = 32 encoder's
// "everything of a chunk in LDS" scheme carries over, and the work is GEMM-shaped and compute-bound in exact f32
// (12 D^2 flop per kept row and step for the update, 2 D^2 per valid edge for the message; 300 GFLOP per 4096-pair
// forward against ~0.3 GB of compulsory traffic per step).  So the path is a short sequence of launches per call, BOTH
// ions in every launch, all of it on a compact row space:
//
//   plan (graph only, once per batch: wide_plan.hip)
//     wide_count      one wave per molecule: kept rows r_b (rows that can send, receive or be pooled - the same rule as
//                     the D = 32 encoders, encoder_plan.hip) and the histogram of valid edges by (ion, bond type)
//     wide_scan       one workgroup: compact row base of every molecule (an ion starts at a multiple of 128 rows),
//                     per-type runs of the type-sorted edge list and their tiles
//     wide_place      valid edges into their type's run (source row per sorted position) and, per kept row, the
//                     positions of its in-edges IN EDGE-SLOT ORDER (the reference's sequential scatter_nd order,
//                     models/layers.py:74-82)
//   run (embed, pool and the prepared images: this file; messages and reduce: wide_message.hip; the update:
//        wide_update.hip, in mode f32x3 wide_update_x3.hip)
//     wide_embed      h[row] = atom_table[atom id]                               (a1)
//     S x  wide_message   m[p] = A[type_p] h[src_p]: one GEMM per type run, 64-edge tiles, the type's matrix resident
//                         in LDS, next tile's rows in flight under the MFMAs      (a2 + a4, models/layers.py:100-117)
//                         (mode f32x3 at D = 128: wide_message_x3 - bf16x9, matrix operands in registers)
//          wide_reduce    agg[row] = sum of its in-edge messages, slot order      (a5); rows with <= 2 in-edges are
//                         left to the update, which adds up to two messages itself (wide_iota + wide_place)
//          wide_update    GatedUpdate on 64-row tiles (two workgroups per CU), [h|agg] and the gate kernels
//                         streamed through LDS in 16-deep k slices, h updated in place (a7, models/layers.py:142-156)
//                         (mode f32x3: wide_update_x3 on 64-row tiles, wide_update_x3b on 128-row tiles once a batch
//                         fills the chip - bf16x9, kernel slices straight from global into LDS)
//     wide_pool       pooled[b] = sum_n h[b,n] [atom_ids[b,n] > 0], ascending n   (a8)
//
// Every product is an exact f32 product on v_mfma_f32_16x16x4_f32; every sum has a fixed order that does not depend
// on where a molecule sits in the batch, so results are bitwise reproducible and independent of sharding.
//
// wide_device.h holds what these files share (limits, workspace layout, parameter blocks, the GatedUpdate arithmetic,
// the LDS opt-in).  Here: what a call runs is decided in one place (choose_launch), and launch_encoder_wide is the list
// above - plan, prepare, embed, S x (message, reduce, update), pool.
#include <climits>
#include <cstdlib>

#include "wide_device.h"

namespace impnn {
namespace wide {

// ------------------------------------------------------------------------------------------------------------
// embed, pool, prepared images
// ------------------------------------------------------------------------------------------------------------
// a1: one wave per molecule (4 in turn), a row per D/4 lanes; an id outside the vocabulary gives a zero row.
__global__ __launch_bounds__(256) void wide_embed_kernel(Inputs in, const int32_t* __restrict__ kept,
                                                         const int32_t* __restrict__ rowbase,
                                                         const float* __restrict__ table, float* __restrict__ h, int D) {
  // one workgroup per molecule, D / 4 threads per row (a wave per molecule and four molecules per wave, as the plan
  // kernels have it, left a batch of 32 pairs with 4 workgroups walking 24 rows each in turn: 23 us)
  const int mol = blockIdx.x;
  const int qd = D >> 2, rpw = 256 / qd;
  const int sub = threadIdx.x / qd, c4 = threadIdx.x - sub * qd;
  const int g = mol >= in.B ? 1 : 0, b = mol - g * in.B;
  const int r = kept[mol], rb = rowbase[mol];
  const int32_t* ids = in.atom_ids[g] + (int64_t)b * in.N;
  for (int n = sub; n < r; n += rpw) {
    const int id = ids[n];
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)id < (unsigned)in.Va) v = ldv4(table + (int64_t)id * D + 4 * c4);
    stv4(h + (int64_t)(rb + n) * D + 4 * c4, v);
  }
}

// a8: one thread per 16-byte piece of a pooled row, 4 rows in flight, ascending n.
__global__ __launch_bounds__(256) void wide_pool_kernel(Inputs in, const int32_t* __restrict__ kept,
                                                        const int32_t* __restrict__ rowbase,
                                                        const float* __restrict__ h, float* __restrict__ pooled0,
                                                        float* __restrict__ pooled1, int D) {
  const int qd = D >> 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t mol = t / qd;
  const int c4 = (int)(t - mol * qd);
  if (mol >= (int64_t)in.n_ions * in.B) return;
  const int g = mol >= in.B ? 1 : 0, b = (int)(mol - (int64_t)g * in.B);
  const int r = kept[mol];
  const int32_t* ids = in.atom_ids[g] + (int64_t)b * in.N;
  const float* src = h + (int64_t)rowbase[mol] * D + 4 * c4;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  int n = 0;
  for (; n + 4 <= r; n += 4) {
    const f32x4_t v0 = ldv4(src + (int64_t)n * D), v1 = ldv4(src + (int64_t)(n + 1) * D);
    const f32x4_t v2 = ldv4(src + (int64_t)(n + 2) * D), v3 = ldv4(src + (int64_t)(n + 3) * D);
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    acc += ids[n] > 0 ? v0 : zero;
    acc += ids[n + 1] > 0 ? v1 : zero;
    acc += ids[n + 2] > 0 ? v2 : zero;
    acc += ids[n + 3] > 0 ? v3 : zero;
  }
  for (; n < r; ++n)
    if (ids[n] > 0) acc += ldv4(src + (int64_t)n * D);
  stv4((g ? pooled1 : pooled0) + (int64_t)b * D + 4 * c4, acc);
}

// The GatedUpdate part of a prepared step: [Wz|Wr] and Wh in slice order [16-k slice][k quad][column][k & 3], then
// the five vectors.  src = the step's canonical weights behind bond_transform (include/impnn.h).
__global__ void wide_gu_image_kernel(const float* __restrict__ src, float* __restrict__ dst, int D) {
  const float* Wz = src;
  const float* bz = Wz + 2 * D * D;
  const float* Wr = bz + D;
  const float* br = Wr + 2 * D * D;
  const float* Wh = br + D;
  const float* bh = Wh + 2 * D * D;
  const float* gamma = bh + D;
  const float* beta = gamma + D;
  const int n1 = 4 * D * D, n2 = 2 * D * D, total = n1 + n2 + 5 * D;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    float v;
    if (t < n1) {
      const int r = t & 3, c = (t >> 2) % (2 * D), qq = ((t >> 2) / (2 * D)) & 3, u = (t >> 2) / (2 * D) >> 2;
      const int k = 16 * u + 4 * qq + r;
      v = c < D ? Wz[k * D + c] : Wr[k * D + c - D];
    } else if (t < n1 + n2) {
      const int s = t - n1;
      const int r = s & 3, c = (s >> 2) % D, qq = ((s >> 2) / D) & 3, u = (s >> 2) / D >> 2;
      v = Wh[(16 * u + 4 * qq + r) * D + c];
    } else {
      const int s = t - n1 - n2, which = s / D, f = s - which * D;
      const float* vec = which == 0 ? bz : which == 1 ? br : which == 2 ? bh : which == 3 ? gamma : beta;
      v = vec[f];
    }
    dst[t] = v;
  }
}

// The same for mode 3: [Wz|Wr] and Wh as three bf16 planes (w = b0 + b1 + b2 exactly) in 32-k slices of MFMA B-operand
// order [slice][plane][k octet][column][8 k] (16-byte units: a lane's operand of one v_mfma_f32_16x16x32_bf16), then the
// five f32 vectors.
__global__ void wide_gu_image_x3_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int D) {
  const float* Wz = src;
  const float* bz = Wz + 2 * D * D;
  const float* Wr = bz + D;
  const float* br = Wr + 2 * D * D;
  const float* Wh = br + D;
  const float* bh = Wh + 2 * D * D;
  const float* gamma = bh + D;
  const float* beta = gamma + D;
  const int NS = D / 16;                    // 32-k slices of a 2D-deep GEMM
  const int n1 = 2 * D * 2 * D, n2 = 2 * D * D;  // weights of [Wz|Wr], of Wh
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n1 + n2; t += gridDim.x * blockDim.x) {
    const bool first = t < n1;
    const int e = first ? t : t - n1, ncol = first ? 2 * D : D;
    // e = ((u * 4 + kq) * ncol + col) * 8 + j   (plane-independent index inside a slice's plane)
    const int j = e & 7, col = (e >> 3) % ncol, kq = ((e >> 3) / ncol) & 3, u = ((e >> 3) / ncol) >> 2;
    const int k = 32 * u + 8 * kq + j;
    const float w = first ? (col < D ? Wz[k * D + col] : Wr[k * D + col - D]) : Wh[k * D + col];
    const unsigned u0 = __float_as_uint(w) & 0xffff0000u;
    const float r1 = w - __uint_as_float(u0);
    const unsigned u1 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(u1);
    const unsigned u2 = __float_as_uint(r2);  // <= 8 significant bits left: its low half is zero
    const size_t plane = (size_t)4 * ncol * 8;                   // bf16 elements of one plane of a slice
    const size_t base = (first ? 0 : (size_t)NS * 3 * 4 * 2 * D * 8) + (size_t)u * 3 * plane + ((size_t)kq * ncol + col) * 8 + j;
    dst[base] = (unsigned short)(u0 >> 16);
    dst[base + plane] = (unsigned short)(u1 >> 16);
    dst[base + 2 * plane] = (unsigned short)(u2 >> 16);
  }
  float* vec = reinterpret_cast<float*>(dst + (size_t)NS * 3 * 4 * 3 * D * 8);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < 5 * D; t += gridDim.x * blockDim.x) {
    const int which = t / D, f = t - which * D;
    const float* v = which == 0 ? bz : which == 1 ? br : which == 2 ? bh : which == 3 ? gamma : beta;
    vec[t] = v[f];
  }
}

// Mode 3: the step's type matrices A[v] (D x D, row-major [feature][k]) once more as three bf16 planes in the operand
// order of wide_message_x3_kernel: per type 16-byte units [plane][k block][k octet][feature] of 8 consecutive k.
__global__ void wide_mat_planes_kernel(const float* __restrict__ mats, unsigned short* __restrict__ dst, int Vb, int D) {
  const int KB = D / 32;
  const size_t per = (size_t)D * D, total = (size_t)Vb * per;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const size_t v = t / per;
    const int e = (int)(t - v * per), f = e / D, k = e - f * D;
    const float w = mats[t];
    const unsigned u0 = __float_as_uint(w) & 0xffff0000u;
    const float r1 = w - __uint_as_float(u0);
    const unsigned u1 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(u1);
    const unsigned u2 = __float_as_uint(r2);  // <= 8 significant bits left: its low half is zero
    const int kb = k >> 5, q = (k >> 3) & 3, j = k & 7;
    const size_t plane = (size_t)KB * 4 * D * 8;  // bf16 elements of one plane of a type
    const size_t base = v * 3 * plane + (((size_t)kb * 4 + q) * D + f) * 8 + j;
    dst[base] = (unsigned short)(u0 >> 16);
    dst[base + plane] = (unsigned short)(u1 >> 16);
    dst[base + 2 * plane] = (unsigned short)(u2 >> 16);
  }
}

}  // namespace wide

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
bool encoder_wide_supported(int N, int E, int D, int K, int S, int Vb) {
  using namespace wide;
  return (D == 64 || D == 128) && K >= 1 && S >= 0 && N >= 1 && N <= kMaxN && E >= 0 && E <= kMaxE && Vb >= 1 &&
         Vb <= kMaxVb;
}

size_t encoder_wide_workspace_bytes(int n_ions, int B, int N, int E, int D, int S, int Vb, bool x3) {
  return wide::ws_layout(n_ions, B, N, E, D, S, Vb, x3).total;
}

// Do the kernels' 32-bit indices cover a batch of this shape?  Sorted positions and compact rows are 32-bit indices
// (vmax, rmax), and the update kernels address a row's sources as 32-bit FLOAT offsets from `agg` (wide::agg_off: row
// codes up to rmax, the row of zeros, times D).  While messages are named directly choose_launch (`direct`) bounds more
// than that; with every row's sum in agg (the largest batches) this is the only bound on rmax * D, so it is part of
// the shape coverage: at D = 128 a batch passes it up to 16.7 M rows - 52 427 pairs of the explicit-hydrogen shape
// (N = 160), 209 710 pairs at N = 40.  (Every other row * D product of the wide sources is formed in 64 bits.)
bool encoder_wide_batch_covered(int n_ions, int B, int N, int E, int D, int Vb) {
  const wide::Ws w = wide::ws_layout(n_ions, B, N, E, D, 0, Vb, false);  // rmax and vmax depend on neither S nor the mode
  return w.vmax < INT_MAX && (w.rmax + 1) * (int64_t)D < ((int64_t)1 << 31);
}

size_t encoder_wide_prepared_bytes(int D, int S, int Vb, bool x3) { return wide::prepared_bytes(D, S, Vb, x3); }

int launch_encoder_wide_prepare(const float* weights, const float* bond_table, int D, int K, int S, int Vb, bool x3,
                                void* prepared, hipStream_t s) {
  using namespace wide;
  float* img = static_cast<float*>(prepared);
  const size_t canon = (size_t)impnn_encoder_step_floats(D, K);
  for (int st = 0; st < S; ++st) {
    const float* w = weights + (size_t)st * canon;
    float* dst = img + (size_t)st * step_floats(D, Vb, x3);
    if (int rc = launch_bond_type_matrices(bond_table, w, dst, Vb, K, D, s)) return rc;
    if (x3) {
      wide_gu_image_x3_kernel<<<128, 256, 0, s>>>(w + (size_t)K * D * D,
                                                  reinterpret_cast<unsigned short*>(dst + (size_t)Vb * D * D), D);
      wide_mat_planes_kernel<<<512, 256, 0, s>>>(dst, reinterpret_cast<unsigned short*>(dst + mat_planes_off(D, Vb)), Vb, D);
    }
    else
      wide_gu_image_kernel<<<64, 256, 0, s>>>(w + (size_t)K * D * D, dst + (size_t)Vb * D * D, D);
    if (int rc = check_launch("encoder_wide_prepare")) return rc;
  }
  return IMPNN_OK;
}

namespace {

// What a call runs, as a function of its shape, its mode and the CUs of the device - and of the three diagnostics
// overrides, each read once per process (impnn.h: results depend on the arguments only).
wide::LaunchChoice choose_launch(const EncoderArgs& a, const wide::Ws& w, int cus) {
  using namespace wide;
  struct Overrides {
    bool no_direct;  // IMPNN_WIDE_NO_DIRECT=1: every row's sum in agg (the other source path, for the tests)
    int tile_rows;   // IMPNN_WIDE_TILE_ROWS: 16 / 32, anything else but 0 = kRT; 0 or unset = the choice below
    int x3_big;      // IMPNN_WIDE_X3_BIG: >= 0 forces big_tiles in mode 3 (0 = off); unset = the choice below
  };
  static const Overrides env = [] {
    const char* nd = getenv("IMPNN_WIDE_NO_DIRECT");
    const char* tr = getenv("IMPNN_WIDE_TILE_ROWS");
    const char* xb = getenv("IMPNN_WIDE_X3_BIG");
    return Overrides{nd && atoi(nd) != 0, tr ? atoi(tr) : 0, xb ? atoi(xb) : -1};
  }();
  const bool x3 = a.mode == 3;
  const int mols = a.n_ions * a.B, nt = a.D / 16;
  constexpr int R = kRT;
  LaunchChoice c{};
  c.mpw = mols <= 1024 ? 1 : kMolPerWg / 4;
  c.mol_wgs = (mols + 4 * c.mpw - 1) / (4 * c.mpw);
  c.te = tile_edges(a.D);
  // May the update kernels name messages directly as a row's sources (32-bit float offsets from `agg`)?  Not where the
  // message buffer lies beyond that range (~70 000 pairs at D = 128); IMPNN_WIDE_NO_DIRECT=1 (diagnostics, read once per
  // process) forces the other path - every row's sum in agg - for the tests.
  // (the update kernels address a row's two sources as 32-bit float offsets from `agg`: batches whose message buffer
  //  lies beyond that range - ~70 000 pairs at D = 128 - keep every row's sum in agg)
  c.m_off = (int64_t)((w.m - w.agg) / 4);
  c.direct = !env.no_direct && c.m_off + (int64_t)w.vmax * a.D < ((int64_t)1 << 31);
  // mode 3: the messages on the bf16 pipe too (the choice depends on the shape only, so a batch and its shards run the
  // same kernels)
  c.x3_msg = x3 && ((nt == 8 && c.te == 64) || (nt == 4 && c.te == 128));
  // update tiles: kRT rows, or 16 rows for batches of up to ~100 pairs (the kept rows are only known on the device: the
  // choice goes by the upper bound mols * N)
  // (only while the smaller tiles still fit one round of two workgroups per CU: a tile's cost is mostly its 48 weight
  //  slices and barriers, not its rows - at 256 pairs 16-row tiles took 666 us per forward against 526 us)
  const int64_t max_tiles = ((int64_t)mols * a.N + R - 1) / R;
  c.tile_rows = 4 * max_tiles <= 2 * cus ? 16 : R;  // (32-row tiles: 574 us at 200 pairs against ~500 us)
  if (env.tile_rows) c.tile_rows = env.tile_rows == 16 ? 16 : (env.tile_rows == 32 ? 32 : R);
  c.gu_grid = (int)(w.rmax / c.tile_rows);
  // mode 3: 128-row tiles once they fill the chip at one workgroup per CU (two rounds and more)
  c.big_tiles = x3 && c.tile_rows == R && (int64_t)mols * a.N >= (int64_t)2 * cus * kRT3;
  if (env.x3_big >= 0) c.big_tiles = x3 && env.x3_big != 0;
  c.tiles_max = (int)(w.rmax / kRT3);
  c.x3b_grid = c.tiles_max + 8 * (cus - 1);
  return c;
}

}  // namespace

int launch_encoder_wide(const EncoderArgs& a, hipStream_t s) {
  using namespace wide;
  const bool x3 = a.mode == 3;
  const Ws w = ws_layout(a.n_ions, a.B, a.N, a.E, a.D, a.S, a.Vb, x3);
  if (!aligned16(a.workspace)) return fail(IMPNN_E_BADARG, "encoder_fused: workspace must be 16B aligned");
  if (!encoder_wide_batch_covered(a.n_ions, a.B, a.N, a.E, a.D, a.Vb))  // (impnn_encoder_workspace_bytes says so first)
    return fail(IMPNN_E_UNSUPPORTED, "encoder_fused: batch of %d pairs x (N=%d, E=%d) at D=%d exceeds 32-bit row / edge "
                "indices or row offsets", a.B, a.N, a.E, a.D);
  char* base = static_cast<char*>(a.workspace);
  auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(base + off); };
  auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  const int cus = device_compute_units();  // persistent message workgroups: one per CU
  const LaunchChoice c = choose_launch(a, w, cus);
  Inputs in{};
  for (int g = 0; g < a.n_ions; ++g) {
    in.atom_ids[g] = a.atom_ids[g];
    in.bond_ids[g] = a.bond_ids[g];
    in.conn[g] = a.conn[g];
  }
  in.n_ions = a.n_ions; in.B = a.B; in.N = a.N; in.E = a.E; in.Va = a.Va; in.Vb = a.Vb;
  in.mpw = c.mpw;
  const int mols = a.n_ions * a.B;
  if (a.phases & 1) {
    launch_wide_plan(in, w, a.workspace, a.D, c, s);
    if (int rc = check_launch("encoder_wide plan")) return rc;
  }
  if (!(a.phases & 2)) return IMPNN_OK;
  if (!aligned16(a.atom_table)) return fail(IMPNN_E_BADARG, "encoder_fused: atom_table must be 16B aligned");
  const float* img[2] = {nullptr, nullptr};
  for (int g = 0; g < a.n_ions && a.S > 0; ++g) {
    if (a.prepared[g]) {
      if (!aligned16(a.prepared[g])) return fail(IMPNN_E_BADARG, "encoder_fused: prepared weights must be 16B aligned");
      img[g] = static_cast<const float*>(a.prepared[g]);
    } else {
      float* dst = reinterpret_cast<float*>(base + w.img + (size_t)g * prepared_bytes(a.D, a.S, a.Vb, x3));
      if (int rc = launch_encoder_wide_prepare(a.weights[g], a.bond_table, a.D, a.K, a.S, a.Vb, x3, dst, s)) return rc;
      img[g] = dst;
    }
  }
  if (a.n_ions == 1) img[1] = img[0];
  profile_record_start(s);
  wide_embed_kernel<<<mols, 256, 0, s>>>(in, I(w.kept), I(w.rowbase), a.atom_table, F(w.h), a.D);
  unsigned long long* stamps = nullptr;  // [gu_grid x 8 | cus x 8] words, the last step's launches win
  {
    size_t sb = 0;
    void* sp = debug_stamp_buffer(&sb);
    if (sp && sb >= ((size_t)c.gu_grid + cus) * 8 * sizeof(unsigned long long)) stamps = static_cast<unsigned long long*>(sp);
  }
  for (int stp = 0; stp < a.S; ++stp) {
    const size_t step_off = (size_t)stp * step_floats(a.D, a.Vb, x3);
    MsgParams mp{};
    mp.h = F(w.h); mp.m = F(w.m);
    mp.img[0] = img[0]; mp.img[1] = img[1];
    mp.mat_off = step_off;
    mp.srcrow = I(w.srcrow); mp.tilebase = I(w.tilebase); mp.meta = I(w.meta);
    mp.nT = w.nT; mp.Vb = a.Vb;
    mp.stamps = stamps ? stamps + (size_t)c.gu_grid * 8 : nullptr;
    mp.planes_off = step_off + mat_planes_off(a.D, a.Vb);
    if (a.E > 0)
      if (int rc = launch_wide_message(mp, a.D, c.te, c.x3_msg, cus, s)) return rc;
    launch_wide_reduce(w, a.workspace, a.n_ions, a.D, c.direct, s);
    GuParams gp{};
    gp.h = F(w.h); gp.agg = F(w.agg);
    gp.c2a = I(w.aggc2); gp.c2b = I(w.aggc2) + w.rmax; gp.m_off = (int)c.m_off;
    gp.img[0] = img[0]; gp.img[1] = img[1];
    gp.gu_off = step_off + (size_t)a.Vb * a.D * a.D;
    gp.meta = I(w.meta); gp.eps = a.ln_eps; gp.n_ions = a.n_ions; gp.tile_rows = c.tile_rows;
    gp.stamps = stamps;
    if (c.big_tiles) {  // batches that fill the chip: 128-row tiles
      gp.cus = cus;
      gp.tiles_max = c.tiles_max;
    }
    if (int rc = x3 ? launch_wide_update_x3(gp, a.D, c.big_tiles, c.big_tiles ? c.x3b_grid : c.gu_grid, s)
                    : launch_wide_update(gp, a.D, c.gu_grid, s))
      return rc;
  }
  const int64_t pool_threads = (int64_t)mols * (a.D / 4);
  wide_pool_kernel<<<(unsigned)((pool_threads + 255) / 256), 256, 0, s>>>(in, I(w.kept), I(w.rowbase), F(w.h),
                                                                         a.pooled[0], a.n_ions > 1 ? a.pooled[1] : nullptr,
                                                                         a.D);
  profile_record_stop(s);
  return check_launch("encoder_wide");
}

}  // namespace impnn
