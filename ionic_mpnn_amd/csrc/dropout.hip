// The dropout counter and mask (include/impnn.h: impnn_dropout_step, impnn_dropout_mask): the step a training pass
// draws its masks at, and the mask the GatedUpdate kernels (layer_kernels.hip, gated_update_bwd.hip) apply to their
// output, as a tensor - the reference's keras Dropout behind the update (models/layers.py:142-156).  The mask is a
// function of (seed, step, layer, row, column) alone (common.h: dropout_bits): no sum, the same bits on every run.
#include "kernel_device.h"

namespace impnn {

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

}  // namespace impnn
