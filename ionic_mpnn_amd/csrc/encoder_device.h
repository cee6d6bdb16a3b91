// Device helpers shared by the fused encoders (encoder_fused.hip: pull form; encoder_typed.hip: per-bond-type form).
#pragma once

#include "encoder_layout.h"

namespace impnn {
namespace enc {
namespace {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Keeps a quad assembled from scalar results in one register tuple (no instruction is emitted): without
// it the compiler splits the following vector arithmetic back into scalar v_add / v_mul.
__device__ __forceinline__ f32x4 as_tuple(f32x4 v) {
  asm("" : "+v"(v));
  return v;
}
// Activations on whole accumulator quads, written as vector arithmetic so that the multiplies / adds
// around the quarter-rate v_exp_f32 / v_rcp_f32 become packed v_pk_{mul,add,fma}_f32 (two lanes of work
// per instruction).  SCALED: the accumulator carries the mode-1 scale kAcc (folded into the constant).
typedef float f32x2 __attribute__((ext_vector_type(2)));
// A splat constant held in an SGPR pair: packed-f32 instructions cannot encode a 32-bit literal, so with a
// literal the compiler falls back to one scalar multiply per element.
__device__ __forceinline__ f32x4 splat_sgpr(float c) {
  f32x2 v = {c, c};
  asm("" : "+s"(v));
  return __builtin_shufflevector(v, v, 0, 1, 0, 1);
}
template <bool SCALED>
__device__ __forceinline__ f32x4 sigmoid4(f32x4 x) {
  const f32x4 a = x * splat_sgpr(SCALED ? -1.44269504088896f / kAcc : -1.44269504088896f);
  f32x4 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = __builtin_amdgcn_exp2f(a[i]);
  const f32x4 d = as_tuple(as_tuple(e) + 1.0f);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_rcpf(d[i]);
  return as_tuple(r);
}
// The same values - the same IEEE operations per element - in single-lane instructions, for mode "f32x3" of the typed
// encoder: beside MFMAs of the bf16 pipe a packed f32 instruction costs a SIMD more issue time than its two scalar
// forms (measured there: -2 % kernel time for the gates, another -2 % for the epilogue; beside the exact-f32 MFMA,
// which takes the vector ALU's own issue slots, the packed forms are the faster ones).  A value that went through
// lane1 lives in a register of its own (no instruction is emitted), so the compiler does not pair neighbouring
// elements up again.
__device__ __forceinline__ float lane1(float v) {
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ f32x4 sigmoid4_lanes(f32x4 x) {
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = __builtin_amdgcn_rcpf(lane1(lane1(__builtin_amdgcn_exp2f(lane1(x[i] * -1.44269504088896f))) + 1.0f));
  return r;
}
__device__ __forceinline__ f32x4 mul4_lanes(f32x4 a, f32x4 b) {
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = lane1(a[i] * b[i]);
  return r;
}
__device__ __forceinline__ f32x4 tanh4_lanes(f32x4 x) {
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = lane1(1.0f -
                 2.0f * __builtin_amdgcn_rcpf(lane1(lane1(__builtin_amdgcn_exp2f(lane1(x[i] * 2.88539008177793f))) + 1.0f)));
  return r;
}
template <bool SCALED>
__device__ __forceinline__ f32x4 tanh4(f32x4 x) {
  const f32x4 a = x * splat_sgpr(SCALED ? 2.88539008177793f / kAcc : 2.88539008177793f);
  f32x4 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = __builtin_amdgcn_exp2f(a[i]);
  const f32x4 d = as_tuple(as_tuple(e) + 1.0f);
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_rcpf(d[i]);
  return 1.0f - 2.0f * as_tuple(r);
}
// s + s[lane ^ 16] + (that sum)[lane ^ 32] in every lane, on the vector ALU: the bits of
//   s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
// (IEEE addition is commutative) without the two LDS round trips of ds_bpermute_b32.  With x = y = s,
// v_permlane16_swap x, y (odd rows of 16 lanes of x <-> even rows of y) leaves x = rows (s0, s0, s2, s2) and
// y = rows (s1, s1, s3, s3); v_permlane32_swap (lanes 32-63 of x <-> lanes 0-31 of y) does the same with the wave's
// halves.  The swaps move only lanes that EXEC enables, so this is for wave-uniform code (EXEC all ones).
// (Inline asm with two named registers: the operands must be two copies of s, which the builtin does not promise.
//  The s_nop covers the VALU-write -> permlane-read wait states the assembler does not insert.)
__device__ __forceinline__ float sum_xor16_xor32(float s) {
  float x = s, y = s;
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
  s = x + y;
  x = s;
  y = s;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
  return x + y;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

}  // namespace
}  // namespace enc
}  // namespace impnn
