// Element types of the caller's tensors at the library's edge (tc_chain_step_typed): float, or bfloat16 / float16 read and
// written as their 16-bit patterns.  Only the loads of the caller's tensors widen and only the stores into them round:
// every kernel in between keeps float32 arithmetic.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <type_traits>

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

}  // namespace tc
