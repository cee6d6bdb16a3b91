// The plan of the wide encoder (encoder_wide.hip has the stage list): wide_iota / wide_count / wide_scan / wide_place.
// Graph only, once per batch.
#include "wide_device.h"

namespace impnn {
namespace wide {

// ------------------------------------------------------------------------------------------------------------
// plan kernels
// ------------------------------------------------------------------------------------------------------------
// Where the GatedUpdate finds a row's aggregated messages: TWO sources per row, c2a[row] + c2b[row] (added where the
// update parks the slice, first slot first: the Reduce's order).  A source is a row of `agg` (code >= 0) or ~position of
// a message in `m`.  A row with one in-edge names that message and the row of zeros at index n of `agg`; a row with two
// names both messages; a row with none the zeros twice; every other row itself (written by wide_reduce) and the zeros.
// wide_reduce then only sums rows with three in-edges and more - the leaves of a tree, every hydrogen of an
// explicit-hydrogen molecule, every chain atom cost neither a read nor a write of an aggregated copy.
// Defaults here, rows with <= 2 in-edges from wide_place.
__global__ void wide_iota_kernel(int32_t* __restrict__ c2a, int32_t* __restrict__ c2b, float* __restrict__ agg, int n,
                                 int D, int32_t* __restrict__ zero, int nz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    c2a[i] = i;
    c2b[i] = n;
  }
  if (i < D) agg[(int64_t)n * D + i] = 0.f;
  if (i < nz) zero[i] = 0;  // meta and the type counters (what wide_zero_kernel did in a launch of its own)
}


// One wave per molecule (4 in turn): kept rows, and the workgroup's histogram of valid edges by (ion, type) - counted
// in LDS, one global atomic per type the workgroup saw.
__global__ __launch_bounds__(256) void wide_count_kernel(Inputs in, int32_t* __restrict__ kept,
                                                         int32_t* __restrict__ cnt) {
  __shared__ int32_t lh[2 * kMaxVb];
  const int nT = in.n_ions * in.Vb;
  for (int t = threadIdx.x; t < nT; t += 256) lh[t] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mols = in.n_ions * in.B;
  for (int i = 0; i < in.mpw; ++i) {
    const int mol = (blockIdx.x * 4 + wave) * in.mpw + i;
    if (mol >= mols) break;
    const int g = mol >= in.B ? 1 : 0, b = mol - g * in.B;
    const int32_t* ids = in.atom_ids[g] + (int64_t)b * in.N;
    int r = 0;
    for (int n = lane; n < in.N; n += 64)
      if (ids[n] > 0) r = n + 1;
    for (int e = lane; e < in.E; e += 64) {
      int sv, tv;
      const int ty = valid_type(in.conn[g], in.bond_ids[g], (int64_t)b * in.E + e, in.N, in.Vb, sv, tv);
      if (ty >= 0) {
        const int mx = (sv > tv ? sv : tv) + 1;
        r = r > mx ? r : mx;
        atomicAdd(&lh[g * in.Vb + ty], 1);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int t = __shfl_xor(r, o);
      r = r > t ? r : t;
    }
    if (lane == 0) kept[mol] = r;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nT; t += 256)
    if (lh[t]) atomicAdd(&cnt[t], lh[t]);
}

// One workgroup of 1024 threads: (a) exclusive scan of the kept rows per ion (an ion's first row is a multiple of kRowAlign),
// (b) per-type runs and tiles.
__global__ __launch_bounds__(1024) void wide_scan_kernel(const int32_t* __restrict__ kept, int32_t* __restrict__ rowbase,
                                                         const int32_t* __restrict__ cnt, int32_t* __restrict__ tstart,
                                                         int32_t* __restrict__ cursor, int32_t* __restrict__ tilebase,
                                                         int32_t* __restrict__ srcrow, int32_t* __restrict__ meta,
                                                         int n_ions, int B, int nT, int te) {
  __shared__ int32_t wsum[16], wsum2[16];
  __shared__ int32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int g = 0; g < n_ions; ++g) {
    const int per = (B + 1023) / 1024;
    const int lo = tid * per, hi = lo + per < B ? lo + per : B;
    int s = 0;
    for (int b = lo; b < hi; ++b) s += kept[g * B + b];
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    int run = base + off + inc - s;
    for (int b = lo; b < hi; ++b) {
      rowbase[g * B + b] = run;
      run += kept[g * B + b];
    }
    if (tid == 1023) carry = off + inc;
    __syncthreads();
    const int rows = carry;
    if (tid == 0) {
      meta[kMetaRows + g] = rows;
      meta[kMetaBase + g] = base;
      meta[kMetaEnd] = base + rows;
    }
    base = (base + rows + kRowAlign - 1) / kRowAlign * kRowAlign;
    __syncthreads();
  }
  {  // types: nT <= 1024, one per thread
    const int c = tid < nT ? cnt[tid] : 0;
    const int tl = (c + te - 1) / te;
    int ic = c, it = tl;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int uc = __shfl_up(ic, o), ut = __shfl_up(it, o);
      if (lane >= o) {
        ic += uc;
        it += ut;
      }
    }
    if (lane == 63) {
      wsum[wave] = ic;
      wsum2[wave] = it;
    }
    __syncthreads();
    int oc = 0, ot = 0;
    for (int w = 0; w < wave; ++w) {
      oc += wsum[w];
      ot += wsum2[w];
    }
    ic += oc;
    it += ot;
    if (tid < nT) {  // a type's run starts at a whole tile: position = te x tile
      tstart[tid] = (it - tl) * te;
      cursor[tid] = (it - tl) * te;
      tilebase[tid] = it - tl;
      // the padding positions behind the run read row 0 in wide_message (any row inside the workspace would do)
      for (int pz = (it - tl) * te + c; pz < it * te; ++pz) srcrow[pz] = 0;
    }
    if (tid == 1023) {  // threads past nT carry zeros: the last inclusive values are the totals
      tstart[nT] = it * te;
      tilebase[nT] = it;
      meta[kMetaValid] = ic;
      meta[kMetaTiles] = it;
    }
  }
}

// Places the valid edges of kMolPerWg molecules: a range per (ion, type) is reserved with one global atomic per
// workgroup, positions inside it come from LDS atomics (where an edge lands inside its run does not matter: nothing
// is summed across sorted positions).  Then, per molecule, the in-edge lists of its kept rows in edge-slot order:
// rowinfo[row] = (first entry, in-degree), entries at the molecule's own E-slot segment of `csr`.
__global__ __launch_bounds__(256) void wide_place_kernel(Inputs in, const int32_t* __restrict__ kept,
                                                         const int32_t* __restrict__ rowbase,
                                                         int32_t* __restrict__ cursor, int32_t* __restrict__ srcrow,
                                                         int2* __restrict__ rowinfo, int32_t* __restrict__ csr,
                                                         int32_t* __restrict__ c2a,
                                                         int32_t* __restrict__ c2b, int zero_row, int direct_ok) {
  __shared__ int32_t lh[2 * kMaxVb];
  __shared__ int16_t tg_s[4][kMaxE];   // target row of a slot, -1 = not a valid edge
  __shared__ int32_t pos_s[4][kMaxE];  // its sorted position
  __shared__ int32_t deg_s[4][kMaxN], off_s[4][kMaxN], cnt_s[4][kMaxN];
  const int nT = in.n_ions * in.Vb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mols = in.n_ions * in.B;
  for (int t = threadIdx.x; t < nT; t += 256) lh[t] = 0;
  __syncthreads();
  for (int i = 0; i < in.mpw; ++i) {
    const int mol = (blockIdx.x * 4 + wave) * in.mpw + i;
    if (mol >= mols) break;
    const int g = mol >= in.B ? 1 : 0, b = mol - g * in.B;
    for (int e = lane; e < in.E; e += 64) {
      int sv, tv;
      const int ty = valid_type(in.conn[g], in.bond_ids[g], (int64_t)b * in.E + e, in.N, in.Vb, sv, tv);
      if (ty >= 0) atomicAdd(&lh[g * in.Vb + ty], 1);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nT; t += 256) {
    const int c = lh[t];
    lh[t] = c ? atomicAdd(&cursor[t], c) : 0;
  }
  __syncthreads();
  for (int i = 0; i < in.mpw; ++i) {
    const int mol = (blockIdx.x * 4 + wave) * in.mpw + i;
    if (mol >= mols) break;
    const int g = mol >= in.B ? 1 : 0, b = mol - g * in.B;
    const int r = kept[mol], rb = rowbase[mol];
    for (int n = lane; n < r; n += 64) deg_s[wave][n] = 0;
    for (int e = lane; e < in.E; e += 64) {
      int sv, tv;
      const int ty = valid_type(in.conn[g], in.bond_ids[g], (int64_t)b * in.E + e, in.N, in.Vb, sv, tv);
      int16_t tg = -1;
      if (ty >= 0) {
        const int p = atomicAdd(&lh[g * in.Vb + ty], 1);
        srcrow[p] = rb + sv;
        pos_s[wave][e] = p;
        tg = (int16_t)tv;
        atomicAdd(&deg_s[wave][tv], 1);
      }
      tg_s[wave][e] = tg;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // this wave's LDS writes and atomics have landed
    __builtin_amdgcn_wave_barrier();
    // exclusive scan of the in-degrees over the kept rows (r <= kMaxN = 4 x 64)
    int run = 0;
    for (int n0 = 0; n0 < r; n0 += 64) {
      const int n = n0 + lane;
      const int d = n < r ? deg_s[wave][n] : 0;
      int inc = d;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
      }
      if (n < r) {
        off_s[wave][n] = run + inc - d;
        rowinfo[rb + n] = make_int2((int)((int64_t)mol * in.E) + run + inc - d, d);
        if (d == 0) c2a[rb + n] = zero_row;  // nothing to add
      }
      run += __shfl(inc, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // slot order inside a row's list: rank = earlier valid slots with the same target = those of earlier 64-slot groups
    // (a running count per target in LDS) + the lower lanes of this group that name the same target (63 readlanes).
    // (Walking all earlier slots per slot was E^2 / 64 LDS reads per lane: 390 us per call at the explicit-hydrogen
    //  shape E = 640, a tenth of the whole encode.)
    for (int n = lane; n < r; n += 64) cnt_s[wave][n] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int e0 = 0; e0 < in.E; e0 += 64) {
      const int e = e0 + lane;
      const int tg = e < in.E ? tg_s[wave][e] : -1;
      int rank = 0;
#pragma unroll
      for (int j = 0; j < 63; ++j) {
        const int tj = __builtin_amdgcn_readlane(tg, j);
        rank += (j < lane && tj == tg) ? 1 : 0;
      }
      if (tg >= 0) {
        rank += cnt_s[wave][tg];
        csr[(int64_t)mol * in.E + off_s[wave][tg] + rank] = pos_s[wave][e];
        const int dg = deg_s[wave][tg];  // (wide_iota_kernel: the sources of rows with one or two in-edges)
        if (dg <= 2 && direct_ok) (rank == 0 ? c2a : c2b)[rb + tg] = ~pos_s[wave][e];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // every lane has read the counts of the earlier groups
      __builtin_amdgcn_wave_barrier();
      if (tg >= 0) atomicAdd(&cnt_s[wave][tg], 1);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

void launch_wide_plan(const Inputs& in, const Ws& w, void* workspace, int D, const LaunchChoice& c, hipStream_t s) {
  char* base = static_cast<char*>(workspace);
  auto I = [&](size_t off) { return reinterpret_cast<int32_t*>(base + off); };
  const int nz = (int)((w.kept - w.meta) / 4);  // meta and the type counters
  wide_iota_kernel<<<(unsigned)(((w.rmax > nz ? w.rmax : nz) + 255) / 256), 256, 0, s>>>(
      I(w.aggc2), I(w.aggc2) + w.rmax, reinterpret_cast<float*>(base + w.agg), (int)w.rmax, D, I(w.meta), nz);
  wide_count_kernel<<<c.mol_wgs, 256, 0, s>>>(in, I(w.kept), I(w.cnt));
  wide_scan_kernel<<<1, 1024, 0, s>>>(I(w.kept), I(w.rowbase), I(w.cnt), I(w.tstart), I(w.cursor), I(w.tilebase),
                                      I(w.srcrow), I(w.meta), in.n_ions, in.B, w.nT, c.te);
  wide_place_kernel<<<c.mol_wgs, 256, 0, s>>>(in, I(w.kept), I(w.rowbase), I(w.cursor), I(w.srcrow),
                                              reinterpret_cast<int2*>(base + w.rowinfo), I(w.csr), I(w.aggc2),
                                              I(w.aggc2) + w.rmax, (int)w.rmax, c.direct ? 1 : 0);
}

}  // namespace wide
}  // namespace impnn
