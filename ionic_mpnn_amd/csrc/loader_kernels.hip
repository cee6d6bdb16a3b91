// Batch assembly on the GPU: the step before the hot path.
//
// The reference builds every batch on the host from Python lists: +1 id shift
// (train_viscosity.py:255-262), a second reverse-edge expansion with [0,0] padding / truncation
// (utils/mp_utils.py:18-45), atom-id padding (utils/mp_utils.py:12-16), np.array(list)[idx]
// (train_viscosity.py:291-314).  Here the id dataset is flattened once into ragged arrays that stay
// resident in HBM, and one launch writes the padded (B,N) / (B,L) / (B,L,2) model inputs of both ions
// for an arbitrary list of sample indices.  Integer copies only: HBM-bound, one wave per (ion, sample),
// every store coalesced.
#include "common.h"

namespace impnn {
namespace {

struct AssembleParams {
  int n_ions, B, M, N, L, shift;
  const int32_t* sample_idx;
  const int32_t* atom_flat[2];
  const int32_t* atom_off[2];
  const int32_t* edge_flat[2];
  const int32_t* bond_flat[2];
  const int32_t* edge_off[2];
  int32_t* atom_ids[2];
  int32_t* bond_ids[2];
  int32_t* conn[2];
  const float* t_flat;
  float* t_out;
};

constexpr int kUnitsPerBlock = 4;

__global__ __launch_bounds__(kUnitsPerBlock* kWave) void batch_assemble_kernel(AssembleParams p) {
  const int unit = blockIdx.x * kUnitsPerBlock + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (unit >= p.n_ions * p.B) return;
  const int g = unit >= p.B ? 1 : 0;
  const int b = unit - g * p.B;
  int s = __builtin_amdgcn_readfirstlane(p.sample_idx[b]);
  const bool present = s >= 0 && s < p.M;  // an index outside the dataset yields an all-padding sample
  if (!present) s = 0;

  const int a0 = __builtin_amdgcn_readfirstlane(p.atom_off[g][s]);
  const int na = present ? min(__builtin_amdgcn_readfirstlane(p.atom_off[g][s + 1]) - a0, p.N) : 0;
  int32_t* arow = p.atom_ids[g] + (size_t)b * p.N;
  for (int n = lane; n < p.N; n += kWave) arow[n] = n < na ? p.atom_flat[g][a0 + n] + p.shift : 0;

  const int e0 = __builtin_amdgcn_readfirstlane(p.edge_off[g][s]);
  const int ne = present ? __builtin_amdgcn_readfirstlane(p.edge_off[g][s + 1]) - e0 : 0;
  const int take = min(2 * ne, p.L);  // slots 2e, 2e+1 = edge e and its reverse; cut at L
  int2* crow = reinterpret_cast<int2*>(p.conn[g]) + (size_t)b * p.L;
  int32_t* brow = p.bond_ids[g] + (size_t)b * p.L;
  const int2* eflat = reinterpret_cast<const int2*>(p.edge_flat[g]);
  for (int j = lane; j < p.L; j += kWave) {
    int2 c = make_int2(0, 0);
    int bd = 0;
    if (j < take) {
      const int2 uv = eflat[e0 + (j >> 1)];
      c = (j & 1) ? make_int2(uv.y, uv.x) : uv;
      bd = p.bond_flat[g][e0 + (j >> 1)] + p.shift;
    }
    crow[j] = c;
    brow[j] = bd;
  }
  if (g == 0 && p.t_out && lane == 0) p.t_out[b] = present ? p.t_flat[s] : 0.0f;
}

// ---------------------------------------------------------------------------------------
// Mini-batch gather from a device-resident, already padded data set (model.fit over the arrays that
// train_viscosity.py:288-314 builds once): rows `rows[r]` of up to 8 tensors -> row r of their batch buffers, one
// launch.  Inside a captured training step this is the first node: the host then only refreshes `rows`.
// ---------------------------------------------------------------------------------------
constexpr int kGatherMax = 8;
struct GatherRows {
  const uint32_t* src[kGatherMax];
  uint32_t* dst[kGatherMax];
  int words[kGatherMax];  // 32-bit words per row
  int n;
};
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherRows g, const int64_t* __restrict__ rows, int n_rows) {
  const int t = blockIdx.y;  // uniform: constant-index selects stay scalar
  const uint32_t* src = g.src[0];
  uint32_t* dst = g.dst[0];
  int words = g.words[0];
#pragma unroll
  for (int q = 1; q < kGatherMax; ++q)
    if (t == q) src = g.src[q], dst = g.dst[q], words = g.words[q];
  for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const uint32_t* s = src + rows[r] * (int64_t)words;
    uint32_t* d = dst + (int64_t)r * words;
    for (int i = threadIdx.x; i < words; i += 256) d[i] = s[i];
  }
}

// ---------------------------------------------------------------------------------------
// Cached frozen steps (data.FrozenStates): out[t][b, :] = table[t][rows[t][b], :] for one or two ions, each with its
// own int32 index and its own row length.  A row is the atom states of one ion, N * D floats (20 KB at N = 160,
// D = 32), so it is cut into pieces of 4 KB: one workgroup per (sample, piece), 256 lanes x one 16-byte load and
// store, the tail piece cut per lane.  The index is read once per workgroup; an index outside the table writes zeros
// and reads nothing.  Row offsets are 64-bit (C * N * D may pass 2^31).
// ---------------------------------------------------------------------------------------
constexpr int kStatePieceFloats = 1024;  // 256 lanes x 4 floats
struct StateRows {
  const float* table[2];
  const int32_t* rows[2];
  float* out[2];
  long long row_floats[2];
  long long table_rows[2];
  int pieces[2];  // ceil(row_floats / kStatePieceFloats)
};
__global__ __launch_bounds__(256) void state_rows_kernel(StateRows g, int pieces_max) {
  const int t = blockIdx.y;  // uniform: constant-index selects stay scalar
  const float* table = t ? g.table[1] : g.table[0];
  const int32_t* rows = t ? g.rows[1] : g.rows[0];
  float* out = t ? g.out[1] : g.out[0];
  const long long row_floats = t ? g.row_floats[1] : g.row_floats[0];
  const long long table_rows = t ? g.table_rows[1] : g.table_rows[0];
  const int pieces = t ? g.pieces[1] : g.pieces[0];
  const int b = blockIdx.x / pieces_max;
  const int piece = blockIdx.x - b * pieces_max;
  if (piece >= pieces) return;  // (the other ion's rows are longer)
  const long long r = rows[b];
  const bool present = r >= 0 && r < table_rows;
  const long long at = (long long)piece * kStatePieceFloats + 4 * (int)threadIdx.x;
  if (at >= row_floats) return;  // the tail piece, per lane (row_floats is a multiple of 4: whole lanes only)
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (present) v = *reinterpret_cast<const float4*>(table + r * row_floats + at);
  *reinterpret_cast<float4*>(out + (long long)b * row_floats + at) = v;
}

}  // namespace

int launch_batch_assemble(int n_ions, const int32_t* sample_idx, int B, int M, const int32_t* const* atom_flat,
                          const int32_t* const* atom_off, const int32_t* const* edge_flat,
                          const int32_t* const* bond_flat, const int32_t* const* edge_off, int shift, int N, int L,
                          int32_t* const* atom_ids, int32_t* const* bond_ids, int32_t* const* conn,
                          const float* t_flat, float* t_out, hipStream_t s) {
  AssembleParams p{};
  p.n_ions = n_ions; p.B = B; p.M = M; p.N = N; p.L = L; p.shift = shift;
  p.sample_idx = sample_idx;
  for (int g = 0; g < n_ions; ++g) {
    p.atom_flat[g] = atom_flat[g]; p.atom_off[g] = atom_off[g]; p.edge_flat[g] = edge_flat[g];
    p.bond_flat[g] = bond_flat[g]; p.edge_off[g] = edge_off[g];
    p.atom_ids[g] = atom_ids[g]; p.bond_ids[g] = bond_ids[g]; p.conn[g] = conn[g];
  }
  p.t_flat = t_flat; p.t_out = t_out;
  const int units = n_ions * B;
  hipLaunchKernelGGL(batch_assemble_kernel, dim3((units + kUnitsPerBlock - 1) / kUnitsPerBlock),
                     dim3(kUnitsPerBlock * kWave), 0, s, p);
  return check_launch("batch_assemble");
}

int launch_gather_rows(int n, const void* const* src, void* const* dst, const int64_t* row_bytes, const int64_t* rows,
                       int n_rows, hipStream_t s) {
  if (n > kGatherMax) return fail(IMPNN_E_UNSUPPORTED, "gather_rows: %d tensors > %d", n, kGatherMax);
  GatherRows g{};
  g.n = n;
  for (int t = 0; t < n; ++t) {
    if (!src[t] || !dst[t]) return fail(IMPNN_E_BADARG, "gather_rows: null tensor %d", t);
    if (row_bytes[t] <= 0 || row_bytes[t] % 4 != 0 || row_bytes[t] / 4 > 0x7fffffff)
      return fail(IMPNN_E_BADARG, "gather_rows: row size of tensor %d must be a positive multiple of 4 bytes", t);
    if ((reinterpret_cast<uintptr_t>(src[t]) | reinterpret_cast<uintptr_t>(dst[t])) & 3u)
      return fail(IMPNN_E_BADARG, "gather_rows: tensor %d is not 4-byte aligned", t);
    g.src[t] = static_cast<const uint32_t*>(src[t]);
    g.dst[t] = static_cast<uint32_t*>(dst[t]);
    g.words[t] = (int)(row_bytes[t] / 4);
  }
  gather_rows_kernel<<<dim3(n_rows < 4096 ? n_rows : 4096, n), 256, 0, s>>>(g, rows, n_rows);
  return check_launch("gather_rows");
}

int launch_state_rows(int n_ions, const float* const* tables, const int32_t* const* rows, float* const* out,
                      const int64_t* row_floats, const int64_t* table_rows, int B, hipStream_t s) {
  StateRows g{};
  int pieces_max = 0;
  for (int t = 0; t < n_ions; ++t) {
    const int64_t pieces = (row_floats[t] + kStatePieceFloats - 1) / kStatePieceFloats;
    if (pieces * B > 0x7fffffff)
      return fail(IMPNN_E_UNSUPPORTED, "state_rows: %lld pieces of ion %d x %d samples exceed one launch",
                  (long long)pieces, t, B);
    g.table[t] = tables[t]; g.rows[t] = rows[t]; g.out[t] = out[t];
    g.row_floats[t] = row_floats[t]; g.table_rows[t] = table_rows[t]; g.pieces[t] = (int)pieces;
    pieces_max = pieces > pieces_max ? (int)pieces : pieces_max;
  }
  state_rows_kernel<<<dim3((unsigned)B * pieces_max, n_ions), 256, 0, s>>>(g, pieces_max);
  return check_launch("state_rows");
}

}  // namespace impnn
