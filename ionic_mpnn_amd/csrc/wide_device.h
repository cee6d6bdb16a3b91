// What more than one source of the wide encoder needs (encoder_wide.hip has the stage list): the limits, the workspace
// layout, the kernels' parameter blocks, the GatedUpdate arithmetic every update kernel shares, the LDS opt-in and the
// per-file launchers (wide_plan.hip, wide_message.hip, wide_update.hip, wide_update_x3.hip).
#pragma once

#include <atomic>

#include "kernel_device.h"

namespace impnn {
namespace wide {

constexpr int kRT = 64;        // rows of a GatedUpdate tile (the exact-f32 kernel; mode 3's large-batch kernel: 128)
constexpr int kRowAlign = 128; // an ion's rows start at a multiple of it (a tile never holds rows of two ions)
constexpr int kMaxN = 256;     // atoms per molecule (LDS tables of wide_place)
constexpr int kMaxE = 1024;    // edge slots per molecule (LDS tables of wide_place; the explicit-hydrogen data sets pad to E = 4 max_bonds = 640)
constexpr int kMaxVb = 512;    // bond vocabulary (types of both ions: one per thread of wide_scan)
constexpr int kMolPerWg = 16;  // molecules of a wide_count / wide_place workgroup (4 waves x 4); launches of up to
                               // 1024 molecules take one molecule per wave (Inputs::mpw: latency, not atomics, bounds them)

// meta words (device): rows of ion g, first compact row of ion g, valid edges, message tiles
enum { kMetaRows = 0, kMetaBase = 2, kMetaEnd = 4, kMetaValid = 5, kMetaTiles = 6, kMetaWords = 16 };

// (the wide encoder's own: layer_kernels.hip leaves the contraction of 1 - 2 rcp(..) to the compiler, this one spells
//  the fused multiply-add out - the two do not compile to the same instructions)
__device__ __forceinline__ float ftanh(float x) {
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008177793f * x)), 1.0f);
}
// The elementwise arithmetic of the GatedUpdate, shared by every update kernel of the wide encoder with the fusion of
// multiply and add spelled out: a batch and its shards may run different kernels (tile sizes) and must agree bit for bit,
// which they do not if the compiler is left to contract `a * b + c` one way in one kernel and another way in the next.
__device__ __forceinline__ float gu_rh(float r_pre, float h) {  // sigmoid(r) * h (models/layers.py:147-148)
#pragma clang fp contract(off)
  return fsig(r_pre) * h;
}
__device__ __forceinline__ float gu_blend(float z, float h, float t_pre) {  // (1 - z) h + z tanh(t) (models/layers.py:150)
#pragma clang fp contract(off)
  const float keep = (1.0f - z) * h;
  return fmaf(z, ftanh(t_pre), keep);
}
__device__ __forceinline__ float gu_inv_std(float sq_dev_sum, float inv_d, float eps) {  // 1 / sqrt(var + eps): v_rsq_f32, 1 ulp
  return __builtin_amdgcn_rsqf(fmaf(sq_dev_sum, inv_d, eps));
}
__device__ __forceinline__ float gu_out(float x, float mean, float inv, float gamma, float beta, float h) {  // LayerNorm + residual
#pragma clang fp contract(off)
  const float n = (x - mean) * inv;
  return fmaf(n, gamma, beta) + h;
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;  // destination of global_load_lds (a wave-uniform LDS address)

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// In-kernel stamps (diagnostics builds only; tools/wide_stamps.py): thread 0 of a workgroup writes s_memtime into
// word `slot` of its 8-word record.  In the product build the macro is empty and no stamp executes.
#ifdef IMPNN_DIAG_WIDE_STAMPS
#define WIDE_STAMP(buf, slot)                                                                     \
  do {                                                                                            \
    if ((buf) && threadIdx.x == 0) (buf)[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#define WIDE_STAMP_REAL(buf, slot)                                                                    \
  do {                                                                                                \
    if ((buf) && threadIdx.x == 0) (buf)[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define WIDE_STAMP(buf, slot) do { } while (0)
#define WIDE_STAMP_REAL(buf, slot) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------------------
struct Ws {
  size_t meta, kept, rowbase, cnt, tstart, tilebase, cursor, srcrow, rowinfo, csr, aggc2, h, agg, m, img, total;
  int64_t rmax, vmax;
  int nT;
};

inline int tile_edges(int D) { return D >= 128 ? 64 : 128; }

// floats of one step of a prepared image: Vb type matrices (D x D, row-major [i][j]) | [Wz|Wr] slices | Wh slices |
// bz br bh gamma beta
// (mode 3: the gate kernels as three bf16 planes: 9 D^2 floats' worth of bytes instead of 6 D^2, and behind the vectors
//  the type matrices once more as three bf16 planes in MFMA operand order: 1.5 Vb D^2 floats' worth - mat_planes_off)
inline size_t mat_planes_off(int D, int Vb) { return (size_t)Vb * D * D + 9 * (size_t)D * D + 5 * (size_t)D; }
inline size_t step_floats(int D, int Vb, bool x3 = false) {
  return x3 ? mat_planes_off(D, Vb) + (size_t)Vb * D * D / 2 * 3 : (size_t)Vb * D * D + 6 * (size_t)D * D + 5 * (size_t)D;
}
inline size_t prepared_bytes(int D, int S, int Vb, bool x3 = false) {
  return align_up((size_t)(S > 0 ? S : 1) * step_floats(D, Vb, x3) * 4, 256);
}

inline Ws ws_layout(int n_ions, int B, int N, int E, int D, int S, int Vb, bool x3 = false) {
  Ws w{};
  const int64_t mols = (int64_t)n_ions * B;
  w.nT = n_ions * Vb;
  w.rmax = (mols * N + (int64_t)n_ions * kRowAlign + kRowAlign - 1) / kRowAlign * kRowAlign;  // whole tiles
  w.vmax = mols * E + (int64_t)(w.nT + 2) * tile_edges(D);  // a type's run is padded to whole tiles
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
  };
  w.meta = take(kMetaWords * 4);
  w.cnt = take((size_t)(w.nT + 1) * 4);  // (meta and cnt are zeroed together)
  w.kept = take((size_t)mols * 4);
  w.rowbase = take((size_t)mols * 4);
  w.tstart = take((size_t)(w.nT + 1) * 4);
  w.tilebase = take((size_t)(w.nT + 1) * 4);
  w.cursor = take((size_t)(w.nT + 1) * 4);
  w.srcrow = take((size_t)w.vmax * 4);
  w.rowinfo = take((size_t)w.rmax * 8);
  w.csr = take((size_t)w.vmax * 4);
  w.aggc2 = take((size_t)w.rmax * 8);  // two sources per row (wide_iota_kernel)
  w.h = take((size_t)w.rmax * D * 4);
  w.agg = take((size_t)(w.rmax + 1) * D * 4);  // + a row of zeros at index rmax
  w.m = take((size_t)w.vmax * D * 4);
  w.img = take((size_t)n_ions * prepared_bytes(D, S, Vb, x3));
  w.total = o;
  return w;
}

struct Inputs {
  const int32_t* atom_ids[2];
  const int32_t* bond_ids[2];
  const int32_t* conn[2];
  int n_ions, B, N, E, Va, Vb;
  int mpw;  // molecules per wave of wide_count / wide_place: kMolPerWg / 4, or 1 for small launches
};

__device__ __forceinline__ int valid_type(const int32_t* conn, const int32_t* bond_ids, int64_t be, int N, int Vb,
                                          int& src, int& tgt) {
  src = conn[be * 2];
  tgt = conn[be * 2 + 1];
  const int ty = bond_ids[be];
  return (src > 0 && tgt > 0 && src < N && tgt < N && (unsigned)ty < (unsigned)Vb) ? ty : -1;
}

// ------------------------------------------------------------------------------------------------------------
// parameter blocks of the run kernels
// ------------------------------------------------------------------------------------------------------------
struct MsgParams {
  const float* h;
  float* m;
  const float* img[2];      // prepared images; the type matrices of this step start at img[g] + mat_off
  size_t mat_off;
  size_t planes_off;        // mode 3: the same matrices as bf16 planes (wide_mat_planes_kernel), img[g] + planes_off
  const int32_t* srcrow;
  const int32_t* tilebase;
  const int32_t* meta;
  int nT, Vb;
  unsigned long long* stamps;  // diagnostics builds only (IMPNN_DIAG_WIDE_STAMPS)
};

// float offset from `agg` of a source of aggregated messages (wide_iota_kernel): a row of agg, or ~position of a message
__device__ __forceinline__ int agg_off(int code, int m_off, int D) { return code >= 0 ? code * D : m_off + (~code) * D; }

struct GuParams {
  float* h;
  const float* agg;
  const int32_t* c2a;        // two sources of aggregated messages per row (wide_iota_kernel)
  const int32_t* c2b;
  int m_off;                 // floats from agg to m (both in one workspace; the launch checks the range)
  const float* img[2];  // the step's GatedUpdate image starts at img[g] + gu_off
  size_t gu_off;
  const int32_t* meta;
  float eps;
  int n_ions;
  int tile_rows;  // rows a workgroup updates: kRT, or 16 for launches too small to fill the chip with kRT-row tiles
  int cus, tiles_max;  // wide_update_x3b_kernel: CUs of the device, 128-row tiles of the row space
  unsigned long long* stamps;  // diagnostics builds only (IMPNN_DIAG_WIDE_STAMPS)
};

constexpr int kRT3 = 128;  // rows of a tile of wide_update_x3b_kernel (mode 3, batches that fill the chip)

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// Dynamic-LDS opt-in above 64 KB, once per (kernel, device): the state is keyed by the kernel itself.
template <auto Kern>
int raise_lds(size_t bytes) {
  if (bytes <= 64 * 1024) return IMPNN_OK;
  static std::atomic<uint64_t> done{0};  // one instance per kernel instantiation
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  const uint64_t bit = 1ull << dev;
  if (done.load(std::memory_order_acquire) & bit) return IMPNN_OK;
  hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return fail(IMPNN_E_LAUNCH, "encoder_wide: cannot raise the LDS limit: %s", hipGetErrorString(e));
  done.fetch_or(bit, std::memory_order_release);
  return IMPNN_OK;
}

// What launch_encoder_wide decides for a batch before it launches anything (encoder_wide.hip: choose_launch).
struct LaunchChoice {
  int mpw, mol_wgs;       // wide_count / wide_place: molecules per wave (Inputs::mpw) and workgroups
  int te;                 // edges of a message tile
  bool direct;            // rows with <= 2 in-edges name their messages as the update's sources (wide_place, wide_reduce)
  bool x3_msg;            // mode 3: the messages on the bf16 pipe
  int tile_rows, gu_grid; // rows of an update tile (16 / 32 / kRT) and the tiles of the row space
  bool big_tiles;         // mode 3: wide_update_x3b_kernel on kRT3-row tiles
  int tiles_max, x3b_grid;  // ... its tiles of the row space and its grid (GuParams::tiles_max)
  int64_t m_off;          // floats from agg to m (GuParams::m_off)
};

// The launchers of the stage files.  Each picks its kernel's instantiation for D (D / 16 = 4 or 8 feature tiles) and owns
// the thread count, the LDS bytes and the LDS opt-in of its kernels; the int ones return an IMPNN_* code.
void launch_wide_plan(const Inputs& in, const Ws& w, void* workspace, int D, const LaunchChoice& c, hipStream_t s);
int launch_wide_message(const MsgParams& p, int D, int te, bool x3_msg, int cus, hipStream_t s);
void launch_wide_reduce(const Ws& w, void* workspace, int n_ions, int D, bool direct, hipStream_t s);
int launch_wide_update(const GuParams& p, int D, int grid, hipStream_t s);              // exact f32; 16-row tiles: the small kernel
int launch_wide_update_x3(const GuParams& p, int D, bool big_tiles, int grid, hipStream_t s);  // mode 3

}  // namespace wide
}  // namespace impnn
