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

// f(Tag<E>) with E the element type of a runtime TC_DTYPE_*; F32 false: the 16-bit types only
template <typename E>
struct Tag {
  using type = E;
};
template <bool F32 = true, typename F>
int with_elem(int dtype, F f) {
  if constexpr (F32)
    if (dtype == TC_DTYPE_F32) return f(Tag<float>{});
  if (dtype == TC_DTYPE_BF16) return f(Tag<__hip_bfloat16>{});
  if (dtype == TC_DTYPE_F16) return f(Tag<__half>{});
  return TC_ERR_INVALID_ARGUMENT;
}

inline bool aligned(const void *p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// f(std::bool_constant...) of runtime bools: the template arguments of a kernel picked at its launch
template <typename F>
void with_bools(F f) {
  f();
}
template <typename F, typename... B>
void with_bools(F f, bool b, B... rest) {
  if (b)
    with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else
    with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// The element functions of the passes that write a gradient last (layout_kernels.hip, layout_rows_kernels.hip).  One
// definition: a step returns the same bits in every layout because every such pass forms its elements with these
// statements.

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

// What a last pass does to an element v on its way out, in float32 (w: the factor of its row, y: its network output)
//   kCopy  : nothing (the xent gradient, or values an earlier stage of the pass made final)
//   kScale : scale * v
//   kWeigh : (scale * w) * v
// PEN (kScale / kWeigh): penalize(scale * v, y, c2), then times w -- the penalty precedes the weight, so the one factor
// of kWeigh cannot be formed.  F32: the value is stored as float32; otherwise it is rounded to 16 bits next, and the
// product is kept a float32 value (weigh).  A pass whose values carry their sign already passes scale = 1.0f, which
// folds away.
enum ScatterMode { kCopy = 0, kScale, kWeigh };
template <int MODE, bool PEN, bool F32>
__device__ __forceinline__ float last_elem(float v, float y, float w, float scale, float c2) {
  static_assert(!(PEN && MODE == kCopy), "the penalty acts on the scaled MMI gradient");
  if constexpr (MODE == kCopy) {
    return v;
  } else if constexpr (PEN) {
    const float g = penalize(scale * v, y, c2);
    return MODE == kWeigh ? weigh(w, g) : g;
  } else if constexpr (MODE == kWeigh) {
    const float f = scale * w;  // (the one factor of the element)
    return F32 ? f * v : weigh(f, v);
  } else {
    // (16-bit: a float32 product on every path -- left to the backend, an element-wise path alone would fuse it into
    // v_fma_mixlo_f16, whose + 0 addend turns a product of -0 into +0)
    return F32 ? scale * v : weigh(scale, v);
  }
}

// What a penalised pass takes beyond its plain form: the network output where the pass's output lies (stride: of its
// rows, where the pass has rows) and c2 = fl32(2c).  Without the penalty it is empty and takes no kernel argument.
template <bool PEN, typename Y>
struct PenArgs {
  const Y *y;
  int64_t stride;
  float c2;
};
template <typename Y>
struct PenArgs<false, Y> {
  static constexpr const Y *y = nullptr;
  static constexpr int64_t stride = 0;
  static constexpr float c2 = 0.0f;
};

}  // namespace tc
