// One separately rounded fp32 operation each, for kernels whose contract is fixed to the bit.  (hip's __fmul_rn /
// __fadd_rn are the plain operators compiled under the default contraction mode: a product and a sum made of them may
// still meet in one fma.  These carry no such leave.)  rn_div and rn_sqrt are the correctly rounded forms: under the
// project's flags `a / b` is the v_div_scale / v_div_fmas / v_div_fixup sequence and sqrtf is v_sqrt_f32 with its
// correction steps, never the approximate reciprocal or square root alone.
#pragma once
#include <hip/hip_runtime.h>

namespace tony {

__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float rn_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}
__device__ __forceinline__ float rn_sqrt(float a) {
#pragma clang fp contract(off)
  return __builtin_sqrtf(a);
}

}  // namespace tony
