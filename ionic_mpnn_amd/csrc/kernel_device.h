// Device and launch helpers shared by train_kernels.hip and message_typed.hip.
#pragma once

#include "common.h"

namespace impnn {
namespace {

constexpr int kBlock = 256;

typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4_t ldv4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
__device__ __forceinline__ void stv4(float* p, f32x4_t v) { *reinterpret_cast<f32x4_t*>(p) = v; }
__device__ __forceinline__ f32x4_t mfma_f32(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

inline int grid_for(int64_t items, int cap = 256 * 8) {
  int64_t g = (items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

}  // namespace
}  // namespace impnn
