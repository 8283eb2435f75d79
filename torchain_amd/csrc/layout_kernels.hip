// Layout conversion either side of the hot path: the reference's recipe hands
// chain_loss a (B, C, T) tensor and torchain/functions.py:118-125 (`to2d`) turns it into frame-major rows
// with x.permute(2,0,1).contiguous(); on the way back autograd undoes the permutation and
// functions.py:112 negates the gradient -- three more passes over a 629 MB tensor at C3.  These two
// kernels do the forward permutation in one pass and the backward permutation, the negation and the
// xent scale in one pass.  Both are plain HBM-bound transposes through LDS: a workgroup moves a
// [64 channels] x [<= 240 frames] tile of one sequence, reading and writing 256-byte (or longer) runs; the
// backward one reads its 2-D rows with 16-byte loads and writes 8-byte pairs where alignment allows.
// The same two kernels take bfloat16 / float16 (B, C, T) tensors (tc_chain_step_typed): the forward one widens as it
// reads, the backward one rounds once as it writes; the tile in LDS and the scale stay float32.  Two plain streams serve
// 16-bit 2-D tensors: a widening copy of strided rows into a contiguous float32 matrix and a rounding copy back.
#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kTileC = 64, kTileTMax = 240, kLayoutThreads = 512;

// the (B, C, T) side holds E (the caller's tensor), the 2-D side float32 (the step's scratch)
template <bool TO2D, typename E>
struct LayoutIo {
  using in_t = typename std::conditional<TO2D, typename Elem<E>::bits, float>::type;
  using out_t = typename std::conditional<TO2D, float, typename Elem<E>::bits>::type;
};

// TO2D: in (B, C, T) contiguous -> out[(t*B + b) * out_stride + c];  !TO2D: the inverse, times `scale`
// (E = float: the float32 kernels; otherwise TO2D widens each element it reads, !TO2D rounds each one it writes)
// W (!TO2D; tc_chain_step_weighted): times a per-row factor as well, out = (scale * row_w[t*B + b]) * in: the factor is
// loaded once per 2-D row a thread reads and folded in as the tile is filled, so the tile holds final float32 values
template <bool TO2D, bool VEC, typename E = float, bool W = false>
__global__ __launch_bounds__(kLayoutThreads) void layout_kernel(const typename LayoutIo<TO2D, E>::in_t *__restrict__ in,
                                                                typename LayoutIo<TO2D, E>::out_t *__restrict__ out,
                                                                int B, int Cn, int T, int64_t stride2d, float scale,
                                                                const float *__restrict__ row_w) {
  constexpr bool kF32 = std::is_same<E, float>::value;
  static_assert(!(W && TO2D), "row factors are for the way back");
  extern __shared__ float tile[];  // kTileC x (frames of the tile | 1): sized by the launch, several blocks per CU
  const int c0 = blockIdx.x * kTileC, b = blockIdx.y, t0 = blockIdx.z * kTileTMax;
  const int tc = min(kTileTMax, T - t0), nc = min(kTileC, Cn - c0);
  const int pitch = tc | 1;  // odd pitch: the transposed accesses are bank-conflict-free
  const int tid = threadIdx.x;
  if constexpr (TO2D) {
    // read runs of tc floats along t (for tc == T the whole tile is one contiguous block); dword accesses on both
    // sides: 16-byte row stores and 8-byte run loads were measured here and are slower (0.30 vs 0.26 ms at C3)
    if (!kF32 && VEC) {
      // 16-bit runs: one dword = two frames when T is even (every run then starts 4-byte aligned; tc is even too)
      const int half = tc / 2;
      for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
        const int c = idx / half, t = 2 * (idx - c * half);
        const uint32_t v = *reinterpret_cast<const uint32_t *>(in + ((int64_t)b * Cn + c0 + c) * T + t0 + t);
        tile[c * pitch + t] = Elem<E>::widen((uint16_t)(v & 0xFFFFu));
        tile[c * pitch + t + 1] = Elem<E>::widen((uint16_t)(v >> 16));
      }
    } else {
      for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
        const int c = idx / tc, t = idx - c * tc;
        tile[c * pitch + t] = Elem<E>::widen(in[((int64_t)b * Cn + c0 + c) * T + t0 + t]);
      }
    }
    __syncthreads();
    const int cx = tid & (kTileC - 1);
    for (int t = tid / kTileC; t < tc; t += kLayoutThreads / kTileC)
      if (cx < nc) out[((int64_t)(t0 + t) * B + b) * stride2d + c0 + cx] = tile[cx * pitch + t];
  } else {
    // Read side: 16-byte loads when the 2-D rows are 16-byte aligned -- a wave then reads four 256-byte row
    // segments per instruction instead of one (the dword form left this kernel at 41 % of the HBM peak).
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
        if constexpr (W) {
          const float f = scale * row_w[(int64_t)(t0 + t) * B + b];
          v = make_float4(f * v.x, f * v.y, f * v.z, f * v.w);
        }
        tile[(cq + 0) * pitch + t] = v.x;
        tile[(cq + 1) * pitch + t] = v.y;
        tile[(cq + 2) * pitch + t] = v.z;
        tile[(cq + 3) * pitch + t] = v.w;
      }
    } else {
      const int cx = tid & (kTileC - 1);
      for (int t = tid / kTileC; t < tc; t += kLayoutThreads / kTileC)
        if (cx < nc) {
          const float v = in[((int64_t)(t0 + t) * B + b) * stride2d + c0 + cx];
          tile[cx * pitch + t] = W ? (scale * row_w[(int64_t)(t0 + t) * B + b]) * v : v;
        }
    }
    __syncthreads();
    const float s = W ? 1.0f : scale;  // (W: the tile holds the scaled values already)
    if constexpr (!kF32) {
      // Write side of a 16-bit tensor: scale in float32, round once; 8-byte stores (4 frames) when every run starts
      // 8-byte aligned, 4-byte ones (2 frames) when it starts 4-byte aligned
      if (VEC && (T & 3) == 0) {
        const int quad = tc / 4;
        for (int idx = tid; idx < nc * quad; idx += kLayoutThreads) {
          const int c = idx / quad, t = 4 * (idx - c * quad);
          const float *src = tile + c * pitch + t;
          const uint32_t lo = Elem<E>::round(s * src[0]) | ((uint32_t)Elem<E>::round(s * src[1]) << 16);
          const uint32_t hi = Elem<E>::round(s * src[2]) | ((uint32_t)Elem<E>::round(s * src[3]) << 16);
          *reinterpret_cast<uint2 *>(out + ((int64_t)b * Cn + c0 + c) * T + t0 + t) = make_uint2(lo, hi);
        }
      } else if (VEC && (T & 1) == 0) {
        const int half = tc / 2;
        for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
          const int c = idx / half, t = 2 * (idx - c * half);
          const float *src = tile + c * pitch + t;
          *reinterpret_cast<uint32_t *>(out + ((int64_t)b * Cn + c0 + c) * T + t0 + t) =
              Elem<E>::round(s * src[0]) | ((uint32_t)Elem<E>::round(s * src[1]) << 16);
        }
      } else {
        for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
          const int c = idx / tc, t = idx - c * tc;
          out[((int64_t)b * Cn + c0 + c) * T + t0 + t] = Elem<E>::round(s * tile[c * pitch + t]);
        }
      }
    } else {
      // Write side: runs of tc floats per channel; 8-byte stores when every run starts 8-byte aligned
      if (VEC && (T & 1) == 0 && (tc & 1) == 0) {
        const int half = tc / 2;
        for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
          const int c = idx / half, t = 2 * (idx - c * half);
          *reinterpret_cast<float2 *>(out + ((int64_t)b * Cn + c0 + c) * T + t0 + t) =
              make_float2(s * tile[c * pitch + t], s * tile[c * pitch + t + 1]);
        }
      } else {
        for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
          const int c = idx / tc, t = idx - c * tc;
          out[((int64_t)b * Cn + c0 + c) * T + t0 + t] = s * tile[c * pitch + t];
        }
      }
    }
  }
}

// 16-bit 2-D input -> float32: (rows, cols) with `in_stride` -> contiguous (rows, cols), one wave per row at a time.
// VEC: 16-byte loads (8 elements) and two 16-byte stores, when cols and in_stride are multiples of 8 and both bases
// 16-byte aligned.
constexpr int kCastThreads = 256, kCastBlocksMax = 4096;
template <typename E, bool VEC>
__global__ __launch_bounds__(kCastThreads) void widen_rows_kernel(const uint16_t *__restrict__ in, int64_t in_stride,
                                                                  float *__restrict__ out, int64_t rows, int cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kCastThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kCastThreads / 64)) {
    const uint16_t *src = in + r * in_stride;
    float *dst = out + r * cols;
    if (VEC) {
      for (int c = lane * 8; c < cols; c += 64 * 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src + c);
        *reinterpret_cast<float4 *>(dst + c) =
            make_float4(Elem<E>::widen((uint16_t)(v.x & 0xFFFFu)), Elem<E>::widen((uint16_t)(v.x >> 16)),
                        Elem<E>::widen((uint16_t)(v.y & 0xFFFFu)), Elem<E>::widen((uint16_t)(v.y >> 16)));
        *reinterpret_cast<float4 *>(dst + c + 4) =
            make_float4(Elem<E>::widen((uint16_t)(v.z & 0xFFFFu)), Elem<E>::widen((uint16_t)(v.z >> 16)),
                        Elem<E>::widen((uint16_t)(v.w & 0xFFFFu)), Elem<E>::widen((uint16_t)(v.w >> 16)));
      }
    } else {
      for (int c = lane; c < cols; c += 64) dst[c] = Elem<E>::widen(src[c]);
    }
  }
}

// float32 -> 16-bit, n contiguous elements, rounded once.  VEC: two 16-byte loads and one 16-byte store per 8 elements
// (n a multiple of 8, both bases 16-byte aligned; with W, cols a multiple of 8 too).  W (tc_chain_step_weighted): element i
// is row i / cols of a (rows, cols) matrix and is rounded from row_w[row] * in[i].
template <typename E, bool VEC, bool W = false>
__global__ __launch_bounds__(kCastThreads) void round_kernel(const float *__restrict__ in, uint16_t *__restrict__ out,
                                                             int64_t n, const float *__restrict__ row_w, int cols) {
  const int64_t step = (int64_t)gridDim.x * kCastThreads;
  if (VEC) {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n / 8; i += step) {
      float4 a = reinterpret_cast<const float4 *>(in)[2 * i], b = reinterpret_cast<const float4 *>(in)[2 * i + 1];
      if constexpr (W) {
        const float f = row_w[8 * i / cols];  // (the 8 elements lie in one row)
        a = make_float4(weigh(f, a.x), weigh(f, a.y), weigh(f, a.z), weigh(f, a.w));
        b = make_float4(weigh(f, b.x), weigh(f, b.y), weigh(f, b.z), weigh(f, b.w));
      }
      auto pack = [](float lo, float hi) { return (uint32_t)Elem<E>::round(lo) | ((uint32_t)Elem<E>::round(hi) << 16); };
      reinterpret_cast<uint4 *>(out)[i] = make_uint4(pack(a.x, a.y), pack(a.z, a.w), pack(b.x, b.y), pack(b.z, b.w));
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n; i += step)
      out[i] = Elem<E>::round(W ? weigh(row_w[i / cols], in[i]) : in[i]);
  }
}

// a[r][c] *= row_w[r] in place, contiguous float32 (rows, cols), one wave per row at a time (the factor is loaded once per
// row and wave).  VEC: 16-byte loads and stores (cols a multiple of 4, base 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(kCastThreads) void scale_rows_kernel(float *__restrict__ a, int64_t rows, int cols,
                                                                  const float *__restrict__ row_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kCastThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kCastThreads / 64)) {
    const float f = row_w[r];
    float *row = a + r * cols;
    if (VEC) {
      for (int c = lane * 4; c < cols; c += 64 * 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c);
        *reinterpret_cast<float4 *>(row + c) = make_float4(f * v.x, f * v.y, f * v.z, f * v.w);
      }
    } else {
      for (int c = lane; c < cols; c += 64) row[c] = f * row[c];
    }
  }
}

// sum_{r,c} a[r][c] * b[r][c] in double: per-block partials in a fixed order, then one block adds them in
// index order -- deterministic.  [K] TraceMatMat(xent_output, xent_deriv, kTrans), the cross-entropy objective
// Kaldi's chain trainer reports (the reference leaves it as a TODO, torchain/functions.py:88-89).
constexpr int kTraceBlocks = 512, kTraceThreads = 256;
__global__ __launch_bounds__(kTraceThreads) void trace_partial_kernel(const float *__restrict__ a, int64_t a_stride,
                                                                      const float *__restrict__ b, int64_t b_stride,
                                                                      int64_t rows, int cols, double *partial) {
  __shared__ double sh[kTraceThreads];
  double acc = 0.0;
  for (int64_t r = blockIdx.x; r < rows; r += kTraceBlocks) {
    const float *ar = a + r * a_stride, *br = b + r * b_stride;
    float row = 0.f;
    for (int c = threadIdx.x; c < cols; c += kTraceThreads) row = fmaf(ar[c], br[c], row);
    acc += (double)row;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int w = kTraceThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void trace_final_kernel(const double *partial, double *out) {
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kTraceBlocks; ++i) t += partial[i];
    *out = t;
  }
}

}  // namespace

int64_t trace_workspace_bytes() { return (int64_t)kTraceBlocks * 8; }

int launch_trace_mat_mat(const float *a, int64_t a_stride, const float *b, int64_t b_stride, int64_t rows, int cols,
                         double *partial, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(trace_partial_kernel, dim3(kTraceBlocks), dim3(kTraceThreads), 0, stream, a, a_stride, b, b_stride,
                     rows, cols, partial);
  hipLaunchKernelGGL(trace_final_kernel, dim3(1), dim3(64), 0, stream, partial, out);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

namespace {

template <typename E>
int launch_layout_16(bool to2d, const void *in, void *out, int B, int Cn, int T, int64_t stride2d, float scale,
                     hipStream_t stream, const float *row_w = nullptr) {
  count_launch(kCntLayout);
  const dim3 grid((Cn + kTileC - 1) / kTileC, B, (T + kTileTMax - 1) / kTileTMax);
  const size_t lds = sizeof(float) * kTileC * ((size_t)(T < kTileTMax ? T : kTileTMax) | 1);
  if (to2d) {
    const uint16_t *src = static_cast<const uint16_t *>(in);
    float *dst = static_cast<float *>(out);
    if ((T & 1) == 0 && ((uintptr_t)in & 3) == 0)
      hipLaunchKernelGGL((layout_kernel<true, true, E>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d, scale,
                         nullptr);
    else
      hipLaunchKernelGGL((layout_kernel<true, false, E>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d, scale,
                         nullptr);
  } else {
    const float *src = static_cast<const float *>(in);
    uint16_t *dst = static_cast<uint16_t *>(out);
    const bool vec = stride2d % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0;
    if (row_w && vec)
      hipLaunchKernelGGL((layout_kernel<false, true, E, true>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d,
                         scale, row_w);
    else if (row_w)
      hipLaunchKernelGGL((layout_kernel<false, false, E, true>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d,
                         scale, row_w);
    else if (vec)
      hipLaunchKernelGGL((layout_kernel<false, true, E>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d, scale,
                         nullptr);
    else
      hipLaunchKernelGGL((layout_kernel<false, false, E>), grid, dim3(kLayoutThreads), lds, stream, src, dst, B, Cn, T, stride2d, scale,
                         nullptr);
  }
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int cast_blocks(int64_t items) {
  const int64_t b = (items + kCastThreads - 1) / kCastThreads;
  return (int)(b < 1 ? 1 : b > kCastBlocksMax ? kCastBlocksMax : b);
}

template <typename E>
int launch_widen_rows_e(const void *in, int64_t in_stride, float *out, int64_t rows, int cols, hipStream_t stream) {
  const uint16_t *src = static_cast<const uint16_t *>(in);
  const int blocks = cast_blocks(rows * 64);  // (a wave per row)
  if (cols % 8 == 0 && in_stride % 8 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
    hipLaunchKernelGGL((widen_rows_kernel<E, true>), dim3(blocks), dim3(kCastThreads), 0, stream, src, in_stride, out, rows, cols);
  else
    hipLaunchKernelGGL((widen_rows_kernel<E, false>), dim3(blocks), dim3(kCastThreads), 0, stream, src, in_stride, out, rows, cols);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_round_e(const float *in, void *out, int64_t n, hipStream_t stream, const float *row_w, int cols) {
  uint16_t *dst = static_cast<uint16_t *>(out);
  const bool vec = n % 8 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
  if (row_w && vec && cols % 8 == 0)
    hipLaunchKernelGGL((round_kernel<E, true, true>), dim3(cast_blocks(n / 8)), dim3(kCastThreads), 0, stream, in, dst, n, row_w, cols);
  else if (row_w)
    hipLaunchKernelGGL((round_kernel<E, false, true>), dim3(cast_blocks(n)), dim3(kCastThreads), 0, stream, in, dst, n, row_w, cols);
  else if (vec)
    hipLaunchKernelGGL((round_kernel<E, true>), dim3(cast_blocks(n / 8)), dim3(kCastThreads), 0, stream, in, dst, n, nullptr, 0);
  else
    hipLaunchKernelGGL((round_kernel<E, false>), dim3(cast_blocks(n)), dim3(kCastThreads), 0, stream, in, dst, n, nullptr, 0);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

int launch_to2d(int dtype, const void *in_bct, float *out, int B, int Cn, int T, int64_t stride2d, hipStream_t stream) {
  switch (dtype) {
    case TC_DTYPE_F32: return launch_layout(true, static_cast<const float *>(in_bct), out, B, Cn, T, stride2d, 1.0f, stream);
    case TC_DTYPE_BF16: return launch_layout_16<__hip_bfloat16>(true, in_bct, out, B, Cn, T, stride2d, 1.0f, stream);
    case TC_DTYPE_F16: return launch_layout_16<__half>(true, in_bct, out, B, Cn, T, stride2d, 1.0f, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_from2d(int dtype, const float *in, int64_t stride2d, void *out_bct, int B, int Cn, int T, float scale,
                  hipStream_t stream, const float *row_w) {
  switch (dtype) {
    case TC_DTYPE_F32: return launch_layout(false, in, static_cast<float *>(out_bct), B, Cn, T, stride2d, scale, stream, row_w);
    case TC_DTYPE_BF16: return launch_layout_16<__hip_bfloat16>(false, in, out_bct, B, Cn, T, stride2d, scale, stream, row_w);
    case TC_DTYPE_F16: return launch_layout_16<__half>(false, in, out_bct, B, Cn, T, stride2d, scale, stream, row_w);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_widen_rows(int dtype, const void *in, int64_t in_stride, float *out, int64_t rows, int cols, hipStream_t stream) {
  switch (dtype) {
    case TC_DTYPE_BF16: return launch_widen_rows_e<__hip_bfloat16>(in, in_stride, out, rows, cols, stream);
    case TC_DTYPE_F16: return launch_widen_rows_e<__half>(in, in_stride, out, rows, cols, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_round(int dtype, const float *in, void *out, int64_t n, hipStream_t stream, const float *row_w, int cols) {
  if (row_w && cols <= 0) return TC_ERR_INVALID_ARGUMENT;
  switch (dtype) {
    case TC_DTYPE_BF16: return launch_round_e<__hip_bfloat16>(in, out, n, stream, row_w, cols);
    case TC_DTYPE_F16: return launch_round_e<__half>(in, out, n, stream, row_w, cols);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_scale_rows(float *a, int64_t rows, int cols, const float *row_w, hipStream_t stream) {
  if (!a || !row_w || rows <= 0 || cols <= 0) return TC_ERR_INVALID_ARGUMENT;
  const int blocks = cast_blocks(rows * 64);  // (a wave per row)
  if (cols % 4 == 0 && ((uintptr_t)a & 15) == 0)
    hipLaunchKernelGGL((scale_rows_kernel<true>), dim3(blocks), dim3(kCastThreads), 0, stream, a, rows, cols, row_w);
  else
    hipLaunchKernelGGL((scale_rows_kernel<false>), dim3(blocks), dim3(kCastThreads), 0, stream, a, rows, cols, row_w);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_layout(bool to2d, const float *in, float *out, int B, int Cn, int T, int64_t stride2d, float scale,
                  hipStream_t stream, const float *row_w) {
  if (to2d && row_w) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntLayout);
  const dim3 grid((Cn + kTileC - 1) / kTileC, B, (T + kTileTMax - 1) / kTileTMax);
  const size_t lds = sizeof(float) * kTileC * ((size_t)(T < kTileTMax ? T : kTileTMax) | 1);
  // 16-byte path of the 2-D side: rows and base 16-byte aligned, whole float4s of channels in every tile
  const bool vec = stride2d % 4 == 0 && ((uintptr_t)(to2d ? out : in) & 15) == 0 && ((uintptr_t)(to2d ? in : out) & 7) == 0;
  if (to2d)
    hipLaunchKernelGGL((layout_kernel<true, false>), grid, dim3(kLayoutThreads), lds, stream, in, out, B, Cn, T, stride2d, scale,
                       nullptr);
  else if (row_w && vec)
    hipLaunchKernelGGL((layout_kernel<false, true, float, true>), grid, dim3(kLayoutThreads), lds, stream, in, out, B, Cn, T,
                       stride2d, scale, row_w);
  else if (row_w)
    hipLaunchKernelGGL((layout_kernel<false, false, float, true>), grid, dim3(kLayoutThreads), lds, stream, in, out, B, Cn, T,
                       stride2d, scale, row_w);
  else if (vec)
    hipLaunchKernelGGL((layout_kernel<false, true>), grid, dim3(kLayoutThreads), lds, stream, in, out, B, Cn, T, stride2d, scale,
                       nullptr);
  else
    hipLaunchKernelGGL((layout_kernel<false, false>), grid, dim3(kLayoutThreads), lds, stream, in, out, B, Cn, T, stride2d, scale,
                       nullptr);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
