// The out-of-range penalty of tc_chain_step_penalized (after [K] PenalizeOutOfRange, restated in torchain_hip.h): the passes
// that write the MMI gradient last, with g' = g + fl32(2c) * p(y) folded in.  They are the penalised twins of three passes of
// layout_kernels.hip -- the (B, C, T) copy back, the 16-bit rounding pass and the float32 2-D row pass -- kept in a file of
// their own so that a step without the penalty runs the kernels it ran before, instruction for instruction.  All three are
// plain HBM streams: one more read (the network output, at the index the pass writes) and a handful of VALU operations.
#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

// (the tile geometry of layout_kernel and the grid of the cast kernels, layout_kernels.hip)
constexpr int kTileC = 64, kTileTMax = 240, kLayoutThreads = 512;
constexpr int kCastThreads = 256, kCastBlocksMax = 4096;

// (weigh and penalize, the element functions of every pass here, the latter with L = kOutputLimit: half_io.h)

// layout_kernel<false, VEC, E, W> with the penalty: in[(t*B + b) * stride2d + c] (float32) -> out (B, C, T) of E,
//   out = row_w[t*B + b] * penalize(scale * in, y, c2)       (W false: no row factor)
// with y the element of `y_bct`, the caller's (B, C, T) network output, at the output's own index, widened exactly.  The
// tile is filled as layout_kernel fills it and holds the plain values; the factors of the tile's frames follow it in LDS
// (W), and the write side reads y with the width of its stores beside them.
template <bool VEC, typename E, bool W>
__global__ __launch_bounds__(kLayoutThreads) void from2d_penalized_kernel(const float *__restrict__ in,
                                                                          typename Elem<E>::bits *__restrict__ out,
                                                                          const typename Elem<E>::bits *__restrict__ y_bct,
                                                                          int B, int Cn, int T, int64_t stride2d, float scale,
                                                                          float c2, const float *__restrict__ row_w) {
  constexpr bool kF32 = std::is_same<E, float>::value;
  extern __shared__ float tile[];  // kTileC x (frames of the tile | 1), then the frames' factors (W)
  const int c0 = blockIdx.x * kTileC, b = blockIdx.y, t0 = blockIdx.z * kTileTMax;
  const int tc = min(kTileTMax, T - t0), nc = min(kTileC, Cn - c0);
  const int pitch = tc | 1;
  const int tid = threadIdx.x;
  float *wt = tile + kTileC * pitch;
  if (VEC) {
    const int cq = (tid & 15) * 4, tr = tid >> 4;  // 16 threads per row segment, 32 rows per pass
    for (int t = tr; t < tc; t += kLayoutThreads / 16) {
      const float *src = in + ((int64_t)(t0 + t) * B + b) * stride2d + c0 + cq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cq + 3 < nc) {
        v = *reinterpret_cast<const float4 *>(src);
      } else {
        if (cq < nc) v.x = src[0];
        if (cq + 1 < nc) v.y = src[1];
        if (cq + 2 < nc) v.z = src[2];
      }
      tile[(cq + 0) * pitch + t] = v.x;
      tile[(cq + 1) * pitch + t] = v.y;
      tile[(cq + 2) * pitch + t] = v.z;
      tile[(cq + 3) * pitch + t] = v.w;
    }
  } else {
    const int cx = tid & (kTileC - 1);
    for (int t = tid / kTileC; t < tc; t += kLayoutThreads / kTileC)
      if (cx < nc) tile[cx * pitch + t] = in[((int64_t)(t0 + t) * B + b) * stride2d + c0 + cx];
  }
  if constexpr (W)
    for (int t = tid; t < tc; t += kLayoutThreads) wt[t] = row_w[(int64_t)(t0 + t) * B + b];
  __syncthreads();
  // element (c, t) of the tile as it leaves, y its network output
  auto fin = [&](int c, int t, float y) -> float {
    const float v = penalize(scale * tile[c * pitch + t], y, c2);
    return W ? weigh(wt[t], v) : v;
  };
  if constexpr (!kF32) {
    // frames t and t + 1 of channel c, rounded once and packed, from the dword that holds their two outputs
    auto fin2 = [&](int c, int t, uint32_t yv) -> uint32_t {
      return (uint32_t)Elem<E>::round(fin(c, t, Elem<E>::widen((uint16_t)(yv & 0xFFFFu)))) |
             ((uint32_t)Elem<E>::round(fin(c, t + 1, Elem<E>::widen((uint16_t)(yv >> 16)))) << 16);
    };
    // 8-byte accesses (4 frames) when every run starts 8-byte aligned, 4-byte ones (2 frames) when 4-byte aligned
    if (VEC && (T & 3) == 0) {
      const int quad = tc / 4;
      for (int idx = tid; idx < nc * quad; idx += kLayoutThreads) {
        const int c = idx / quad, t = 4 * (idx - c * quad);
        const int64_t at = ((int64_t)b * Cn + c0 + c) * T + t0 + t;
        const uint2 yv = *reinterpret_cast<const uint2 *>(y_bct + at);
        *reinterpret_cast<uint2 *>(out + at) = make_uint2(fin2(c, t, yv.x), fin2(c, t + 2, yv.y));
      }
    } else if (VEC && (T & 1) == 0) {
      const int half = tc / 2;
      for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
        const int c = idx / half, t = 2 * (idx - c * half);
        const int64_t at = ((int64_t)b * Cn + c0 + c) * T + t0 + t;
        *reinterpret_cast<uint32_t *>(out + at) = fin2(c, t, *reinterpret_cast<const uint32_t *>(y_bct + at));
      }
    } else {
      for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
        const int c = idx / tc, t = idx - c * tc;
        const int64_t at = ((int64_t)b * Cn + c0 + c) * T + t0 + t;
        out[at] = Elem<E>::round(fin(c, t, Elem<E>::widen(y_bct[at])));
      }
    }
  } else {
    // runs of tc floats per channel; 8-byte accesses when every run starts 8-byte aligned
    if (VEC && (T & 1) == 0 && (tc & 1) == 0) {
      const int half = tc / 2;
      for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
        const int c = idx / half, t = 2 * (idx - c * half);
        const int64_t at = ((int64_t)b * Cn + c0 + c) * T + t0 + t;
        const float2 yv = *reinterpret_cast<const float2 *>(y_bct + at);
        *reinterpret_cast<float2 *>(out + at) = make_float2(fin(c, t, yv.x), fin(c, t + 1, yv.y));
      }
    } else {
      for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
        const int c = idx / tc, t = idx - c * tc;
        const int64_t at = ((int64_t)b * Cn + c0 + c) * T + t0 + t;
        out[at] = fin(c, t, y_bct[at]);
      }
    }
  }
}

// round_kernel<E, VEC, W> with the penalty: element i of n contiguous floats is rounded once from
// row_w[i / cols] * penalize(in[i], y[i], c2), y the widened network output (n contiguous floats as well).
// VEC: n a multiple of 8, the three bases 16-byte aligned (with W, cols a multiple of 8 too).
template <typename E, bool VEC, bool W>
__global__ __launch_bounds__(kCastThreads) void round_penalized_kernel(const float *__restrict__ in, uint16_t *__restrict__ out,
                                                                       int64_t n, const float *__restrict__ y, float c2,
                                                                       const float *__restrict__ row_w, int cols) {
  const int64_t step = (int64_t)gridDim.x * kCastThreads;
  if (VEC) {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n / 8; i += step) {
      float4 a = reinterpret_cast<const float4 *>(in)[2 * i], b = reinterpret_cast<const float4 *>(in)[2 * i + 1];
      const float4 ya = reinterpret_cast<const float4 *>(y)[2 * i], yb = reinterpret_cast<const float4 *>(y)[2 * i + 1];
      a = make_float4(penalize(a.x, ya.x, c2), penalize(a.y, ya.y, c2), penalize(a.z, ya.z, c2), penalize(a.w, ya.w, c2));
      b = make_float4(penalize(b.x, yb.x, c2), penalize(b.y, yb.y, c2), penalize(b.z, yb.z, c2), penalize(b.w, yb.w, c2));
      if constexpr (W) {
        const float f = row_w[8 * i / cols];  // (the 8 elements lie in one row)
        a = make_float4(weigh(f, a.x), weigh(f, a.y), weigh(f, a.z), weigh(f, a.w));
        b = make_float4(weigh(f, b.x), weigh(f, b.y), weigh(f, b.z), weigh(f, b.w));
      }
      auto pack = [](float lo, float hi) { return (uint32_t)Elem<E>::round(lo) | ((uint32_t)Elem<E>::round(hi) << 16); };
      reinterpret_cast<uint4 *>(out)[i] = make_uint4(pack(a.x, a.y), pack(a.z, a.w), pack(b.x, b.y), pack(b.z, b.w));
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n; i += step) {
      const float v = penalize(in[i], y[i], c2);
      out[i] = Elem<E>::round(W ? weigh(row_w[i / cols], v) : v);
    }
  }
}

// a[r][c] = row_w[r] * penalize(a[r][c], y[r * y_stride + c], c2) in place (W false: no row factor): scale_rows_kernel with
// the penalty in the same pass, one wave per row at a time.  y: the caller's own 2-D network output, read with its row
// stride.  VEC: 16-byte accesses on both (cols and y_stride multiples of 4, both bases 16-byte aligned).
template <bool VEC, bool W>
__global__ __launch_bounds__(kCastThreads) void penalize_rows_kernel(float *__restrict__ a, int64_t rows, int cols,
                                                                     const float *__restrict__ y, int64_t y_stride, float c2,
                                                                     const float *__restrict__ row_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kCastThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kCastThreads / 64)) {
    const float f = W ? row_w[r] : 1.0f;
    float *row = a + r * cols;
    const float *yr = y + r * y_stride;
    if (VEC) {
      for (int c = lane * 4; c < cols; c += 64 * 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c), u = *reinterpret_cast<const float4 *>(yr + c);
        float4 o = make_float4(penalize(v.x, u.x, c2), penalize(v.y, u.y, c2), penalize(v.z, u.z, c2), penalize(v.w, u.w, c2));
        if constexpr (W) o = make_float4(f * o.x, f * o.y, f * o.z, f * o.w);
        *reinterpret_cast<float4 *>(row + c) = o;
      }
    } else {
      for (int c = lane; c < cols; c += 64) {
        const float o = penalize(row[c], yr[c], c2);
        row[c] = W ? f * o : o;
      }
    }
  }
}

int cast_blocks(int64_t items) {
  const int64_t b = (items + kCastThreads - 1) / kCastThreads;
  return (int)(b < 1 ? 1 : b > kCastBlocksMax ? kCastBlocksMax : b);
}

template <typename E>
int launch_from2d_penalized_e(const float *in, int64_t stride2d, void *out_bct, const void *y_bct, int B, int Cn, int T,
                              float scale, float c2, const float *row_w, hipStream_t stream) {
  using bits = typename Elem<E>::bits;
  count_launch(kCntLayout);
  const dim3 grid((Cn + kTileC - 1) / kTileC, B, (T + kTileTMax - 1) / kTileTMax), threads(kLayoutThreads);
  const size_t frames = (size_t)(T < kTileTMax ? T : kTileTMax);
  const size_t lds = sizeof(float) * (kTileC * (frames | 1) + (row_w ? frames : 0));
  bits *out = static_cast<bits *>(out_bct);
  const bits *y = static_cast<const bits *>(y_bct);
  // 16-byte path of the 2-D side and 8-byte accesses of the (B, C, T) side, as launch_layout; y travels with the output
  const bool vec = stride2d % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out_bct & 7) == 0 && ((uintptr_t)y_bct & 7) == 0;
  if (vec && row_w)
    hipLaunchKernelGGL((from2d_penalized_kernel<true, E, true>), grid, threads, lds, stream, in, out, y, B, Cn, T, stride2d, scale,
                       c2, row_w);
  else if (vec)
    hipLaunchKernelGGL((from2d_penalized_kernel<true, E, false>), grid, threads, lds, stream, in, out, y, B, Cn, T, stride2d, scale,
                       c2, row_w);
  else if (row_w)
    hipLaunchKernelGGL((from2d_penalized_kernel<false, E, true>), grid, threads, lds, stream, in, out, y, B, Cn, T, stride2d, scale,
                       c2, row_w);
  else
    hipLaunchKernelGGL((from2d_penalized_kernel<false, E, false>), grid, threads, lds, stream, in, out, y, B, Cn, T, stride2d,
                       scale, c2, row_w);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_round_penalized_e(const float *in, void *out, int64_t n, const float *y, float c2, const float *row_w, int cols,
                             hipStream_t stream) {
  uint16_t *dst = static_cast<uint16_t *>(out);
  const bool vec = n % 8 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
                   (!row_w || cols % 8 == 0);
  const dim3 blocks(cast_blocks(vec ? n / 8 : n)), threads(kCastThreads);
  if (vec && row_w)
    hipLaunchKernelGGL((round_penalized_kernel<E, true, true>), blocks, threads, 0, stream, in, dst, n, y, c2, row_w, cols);
  else if (vec)
    hipLaunchKernelGGL((round_penalized_kernel<E, true, false>), blocks, threads, 0, stream, in, dst, n, y, c2, row_w, cols);
  else if (row_w)
    hipLaunchKernelGGL((round_penalized_kernel<E, false, true>), blocks, threads, 0, stream, in, dst, n, y, c2, row_w, cols);
  else
    hipLaunchKernelGGL((round_penalized_kernel<E, false, false>), blocks, threads, 0, stream, in, dst, n, y, c2, row_w, cols);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

int launch_from2d_penalized(int dtype, const float *in, int64_t stride2d, void *out_bct, const void *y_bct, int B, int Cn,
                            int T, float scale, float pen_c2, const float *row_w, hipStream_t stream) {
  if (!in || !out_bct || !y_bct || B <= 0 || Cn <= 0 || T <= 0 || stride2d < Cn || !(pen_c2 > 0.0f)) return TC_ERR_INVALID_ARGUMENT;
  if (B > 65535 || (T + kTileTMax - 1) / kTileTMax > 65535) return TC_ERR_UNSUPPORTED;  // grid y / z limits
  switch (dtype) {
    case TC_DTYPE_F32: return launch_from2d_penalized_e<float>(in, stride2d, out_bct, y_bct, B, Cn, T, scale, pen_c2, row_w, stream);
    case TC_DTYPE_BF16:
      return launch_from2d_penalized_e<__hip_bfloat16>(in, stride2d, out_bct, y_bct, B, Cn, T, scale, pen_c2, row_w, stream);
    case TC_DTYPE_F16: return launch_from2d_penalized_e<__half>(in, stride2d, out_bct, y_bct, B, Cn, T, scale, pen_c2, row_w, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_round_penalized(int dtype, const float *in, void *out, int64_t n, const float *y, float pen_c2, const float *row_w,
                           int cols, hipStream_t stream) {
  if (!in || !out || !y || n <= 0 || !(pen_c2 > 0.0f) || (row_w && cols <= 0)) return TC_ERR_INVALID_ARGUMENT;
  switch (dtype) {
    case TC_DTYPE_BF16: return launch_round_penalized_e<__hip_bfloat16>(in, out, n, y, pen_c2, row_w, cols, stream);
    case TC_DTYPE_F16: return launch_round_penalized_e<__half>(in, out, n, y, pen_c2, row_w, cols, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_penalize_rows(float *a, int64_t rows, int cols, const float *y, int64_t y_stride, float pen_c2, const float *row_w,
                         hipStream_t stream) {
  if (!a || !y || rows <= 0 || cols <= 0 || y_stride < cols || !(pen_c2 > 0.0f)) return TC_ERR_INVALID_ARGUMENT;
  const dim3 blocks(cast_blocks(rows * 64)), threads(kCastThreads);  // (a wave per row)
  const bool vec = cols % 4 == 0 && y_stride % 4 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)y & 15) == 0;
  if (vec && row_w)
    hipLaunchKernelGGL((penalize_rows_kernel<true, true>), blocks, threads, 0, stream, a, rows, cols, y, y_stride, pen_c2, row_w);
  else if (vec)
    hipLaunchKernelGGL((penalize_rows_kernel<true, false>), blocks, threads, 0, stream, a, rows, cols, y, y_stride, pen_c2, row_w);
  else if (row_w)
    hipLaunchKernelGGL((penalize_rows_kernel<false, true>), blocks, threads, 0, stream, a, rows, cols, y, y_stride, pen_c2, row_w);
  else
    hipLaunchKernelGGL((penalize_rows_kernel<false, false>), blocks, threads, 0, stream, a, rows, cols, y, y_stride, pen_c2, row_w);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
