// Element types of the caller's tensors at the library's edge (tc_chain_step_typed): float, or bfloat16 / float16 read and
// written as their 16-bit patterns.  Only the loads of the caller's tensors widen and only the stores into them round:
// every kernel in between keeps float32 arithmetic.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <type_traits>

#include "chain_internal.h"  // kOutputLimit

namespace tc {

template <typename E>
struct Elem;

template <>
struct Elem<float> {
  using bits = float;
  static __device__ __forceinline__ float widen(float v) { return v; }
};

template <>
struct Elem<__hip_bfloat16> {
  using bits = uint16_t;
  static __device__ __forceinline__ float widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }  // (exact)
  // round to nearest even on the bits, every NaN to 0x7FC0: what torch's float -> bfloat16 cast gives on ROCm (c10
  // round_to_nearest_even), subnormals included.  The hardware conversion keeps a NaN's sign and payload instead.
  static __device__ __forceinline__ uint16_t round(float f) {
    if (f != f) return 0x7FC0;
    const uint32_t u = __float_as_uint(f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
  }
};

template <>
struct Elem<__half> {
  using bits = uint16_t;
  static __device__ __forceinline__ float widen(uint16_t b) { return __half2float(__ushort_as_half(b)); }  // (exact)
  // v_cvt_f16_f32, round to nearest even: the conversion torch's float -> float16 cast makes on the device
  static __device__ __forceinline__ uint16_t round(float f) { return __half_as_ushort(__float2half(f)); }
};

// element i of a caller's tensor of element type E that the library's structures carry as `const float *`
template <typename E>
__device__ __forceinline__ float load_elem(const float *p, int64_t i) {
  return Elem<E>::widen(reinterpret_cast<const typename Elem<E>::bits *>(p)[i]);
}

// The two element functions of the passes that write a gradient last (layout_kernels.hip, penalty_kernels.hip,
// layout_rows_kernels.hip).  One definition: a step returns the same bits in every layout because every such pass
// forms its elements with these statements.

// w * v as a float32 value: the empty asm keeps the backend from fusing the multiply into the float16 conversion
// (v_fma_mixlo_f16 rounds the exact product straight to 16 bits, and its + 0 addend turns a product of -0 into +0)
__device__ __forceinline__ float weigh(float w, float v) {
  float p = w * v;
  asm volatile("" : "+v"(p));
  return p;
}

// g + c2 * p with p = y - L above L, y + L below -L and 0 elsewhere, L = kOutputLimit: a NaN fails both comparisons, +-inf
// is taken out.  The product and the sum are two float32 operations: the empty asm keeps the backend from contracting
// them, or a product that formed g, into an FMA (or the sum into a 16-bit conversion).  An element with p == 0 keeps g's
// bits, a zero's sign included.
__device__ __forceinline__ float penalize(float g, float y, float c2) {
  float p = y > kOutputLimit ? y - kOutputLimit : (y < -kOutputLimit ? y + kOutputLimit : 0.0f);
  p = __builtin_isinf(y) ? 0.0f : p;
  float t = c2 * p;
  asm volatile("" : "+v"(t), "+v"(g));  // (g too: the caller's scale * v must not merge with the sum either)
  float r = g + t;
  asm volatile("" : "+v"(r));
  return p != 0.0f ? r : g;
}

}  // namespace tc
