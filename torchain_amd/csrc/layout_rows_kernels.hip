// Channel-last views at the library's edge (tc_chain_step_strided, TC_LAYOUT_CHANNEL_LAST): a (B, C, T) tensor whose channel
// stride is 1 -- the output of a batch-first LSTM or Transformer passed as out.transpose(1, 2), or one half of a joint head --
// has its element (b, c, t) at b*sb + t*st + c.  Its rows are whole already, so the way in and the way out are row copies with
// a permuted row index, not transposes: no LDS, one wave per row at a time, 16-byte lanes where every address allows them.
//   gather  : y2d[(t*B + b) * stride + c] = widen(x[b*sb + t*st + c])                      (float32 / bfloat16 / float16 in)
//   scatter : out[b*osb + t*ost + c] = round(f(in2d[(t*B + b) * stride + c]))              (float32 in)
// with f exactly what the (B, C, T) copy back computes (layout_kernels.hip: layout_kernel, penalty_kernels.hip:
// from2d_penalized_kernel), operation for operation -- plain scale * v; with row weights (scale * w[row]) * v; with the
// penalty w[row] * penalize(scale * v, y) -- so that a channel-last step returns the bits of the step on the contiguous copy.
// A file of its own: no existing code object changes.
#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kRowsThreads = 256, kRowsBlocksMax = 4096;

// (weigh and penalize, the element functions of the scatter: half_io.h)

// elements a lane moves with one 16-byte access of the caller's tensor: 4 floats or 8 16-bit values
template <typename E>
struct Lane {
  static constexpr int kN = std::is_same<E, float>::value ? 4 : 8;
};

// kN elements of a caller's tensor at a 16-byte aligned address, widened
template <typename E>
__device__ __forceinline__ void load_lane(const typename Elem<E>::bits *p, float (&v)[Lane<E>::kN]) {
  if constexpr (std::is_same<E, float>::value) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    const uint4 q = *reinterpret_cast<const uint4 *>(p);
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = Elem<E>::widen((uint16_t)(d[i] & 0xFFFFu));
      v[2 * i + 1] = Elem<E>::widen((uint16_t)(d[i] >> 16));
    }
  }
}

// kN contiguous floats of the 2-D side (16-byte aligned): one or two 16-byte accesses
template <int N>
__device__ __forceinline__ void load_floats(const float *p, float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p + i);
    v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
  }
}
template <int N>
__device__ __forceinline__ void store_floats(float *p, const float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; i += 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
}

// x[b*sb + t*st + c] (E) -> out[(t*B + b) * out_stride + c] (float32), rows = T * B.
// VEC: cols, sb, st multiples of Lane<E>::kN, out_stride a multiple of 4, both bases 16-byte aligned.
template <typename E, bool VEC>
__global__ __launch_bounds__(kRowsThreads) void rows_gather_kernel(const typename Elem<E>::bits *__restrict__ x, int64_t sb,
                                                                   int64_t st, float *__restrict__ out, int64_t out_stride,
                                                                   int B, int64_t rows, int cols) {
  constexpr int kN = Lane<E>::kN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kRowsThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kRowsThreads / 64)) {
    const int64_t t = r / B, b = r - t * B;
    const typename Elem<E>::bits *src = x + b * sb + t * st;
    float *dst = out + r * out_stride;
    if (VEC) {
      for (int c = lane * kN; c < cols; c += 64 * kN) {
        float v[kN];
        load_lane<E>(src + c, v);
        store_floats<kN>(dst + c, v);
      }
    } else {
      for (int c = lane; c < cols; c += 64) dst[c] = Elem<E>::widen(src[c]);
    }
  }
}

// what the scatter does to an element on its way out
//   kCopy  : nothing (the xent gradient: the numerator wrote final values)
//   kScale : scale * v
//   kWeigh : (scale * row_w[row]) * v
// PEN (kScale / kWeigh): penalize(scale * v, y, c2), then times row_w[row]; y = widen(yx[b*ysb + t*yst + c]), the network
// output at the index the element is written to.
enum ScatterMode { kCopy = 0, kScale, kWeigh };

// in[(t*B + b) * in_stride + c] (float32) -> out[b*osb + t*ost + c] (E), rounded once.
// VEC: cols, osb, ost (PEN: ysb, yst too) multiples of Lane<E>::kN, in_stride a multiple of 4, all bases 16-byte aligned.
template <typename E, bool VEC, int MODE, bool PEN>
__global__ __launch_bounds__(kRowsThreads) void rows_scatter_kernel(const float *__restrict__ in, int64_t in_stride,
                                                                    typename Elem<E>::bits *__restrict__ out, int64_t osb,
                                                                    int64_t ost, const typename Elem<E>::bits *__restrict__ yx,
                                                                    int64_t ysb, int64_t yst, int B, int64_t rows, int cols,
                                                                    float scale, float c2, const float *__restrict__ row_w) {
  static_assert(!(PEN && MODE == kCopy), "the penalty acts on the scaled MMI gradient");
  constexpr bool kF32 = std::is_same<E, float>::value;
  constexpr int kN = Lane<E>::kN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kRowsThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kRowsThreads / 64)) {
    const int64_t t = r / B, b = r - t * B;
    const float *src = in + r * in_stride;
    typename Elem<E>::bits *dst = out + b * osb + t * ost;
    const typename Elem<E>::bits *yr = PEN ? yx + b * ysb + t * yst : nullptr;
    const float w = MODE == kWeigh ? row_w[r] : 1.0f;
    const float f = scale * w;  // (kWeigh without the penalty: the one factor of the element)
    // element as it leaves, in float32
    auto fin = [&](float v, float y) -> float {
      if constexpr (MODE == kCopy) {
        return v;
      } else if constexpr (PEN) {
        const float g = penalize(scale * v, y, c2);
        return MODE == kWeigh ? weigh(w, g) : g;
      } else if constexpr (MODE == kWeigh) {
        return kF32 ? f * v : weigh(f, v);
      } else {
        // (16-bit: a float32 product on every path -- left to the backend, the element-wise path alone would fuse it into
        // v_fma_mixlo_f16, whose + 0 addend turns a product of -0 into +0)
        return kF32 ? scale * v : weigh(scale, v);
      }
    };
    if (VEC) {
      for (int c = lane * kN; c < cols; c += 64 * kN) {
        float v[kN], y[kN] = {};
        load_floats<kN>(src + c, v);
        if constexpr (PEN) load_lane<E>(yr + c, y);
#pragma unroll
        for (int i = 0; i < kN; ++i) v[i] = fin(v[i], y[i]);
        if constexpr (kF32) {
          store_floats<kN>(dst + c, v);
        } else {
          auto pack = [](float lo, float hi) { return (uint32_t)Elem<E>::round(lo) | ((uint32_t)Elem<E>::round(hi) << 16); };
          *reinterpret_cast<uint4 *>(dst + c) = make_uint4(pack(v[0], v[1]), pack(v[2], v[3]), pack(v[4], v[5]), pack(v[6], v[7]));
        }
      }
    } else {
      for (int c = lane; c < cols; c += 64) {
        const float y = PEN ? Elem<E>::widen(yr[c]) : 0.0f;
        const float v = fin(src[c], y);
        if constexpr (kF32)
          dst[c] = v;
        else
          dst[c] = Elem<E>::round(v);
      }
    }
  }
}

int rows_blocks(int64_t rows) {
  const int64_t b = (rows + kRowsThreads / 64 - 1) / (kRowsThreads / 64);  // (a wave per row)
  return (int)(b < 1 ? 1 : b > kRowsBlocksMax ? kRowsBlocksMax : b);
}

bool aligned(const void *p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

template <typename E>
int launch_rows_gather_e(const void *x_v, int64_t sb, int64_t st, float *out, int64_t out_stride, int B, int T, int cols,
                         hipStream_t stream) {
  using bits = typename Elem<E>::bits;
  constexpr int kN = Lane<E>::kN;
  const bits *x = static_cast<const bits *>(x_v);
  const int64_t rows = (int64_t)B * T;
  const dim3 blocks(rows_blocks(rows)), threads(kRowsThreads);
  // (a stride of a size-1 dimension is never multiplied by anything but 0)
  const bool vec = cols % kN == 0 && (B == 1 || sb % kN == 0) && (T == 1 || st % kN == 0) && out_stride % 4 == 0 &&
                   aligned(x_v, 16) && aligned(out, 16);
  if (vec)
    hipLaunchKernelGGL((rows_gather_kernel<E, true>), blocks, threads, 0, stream, x, sb, st, out, out_stride, B, rows, cols);
  else
    hipLaunchKernelGGL((rows_gather_kernel<E, false>), blocks, threads, 0, stream, x, sb, st, out, out_stride, B, rows, cols);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E, bool VEC>
void launch_rows_scatter_v(int mode, bool pen, dim3 blocks, hipStream_t stream, const float *in, int64_t in_stride,
                           typename Elem<E>::bits *out, int64_t osb, int64_t ost, const typename Elem<E>::bits *y, int64_t ysb,
                           int64_t yst, int B, int64_t rows, int cols, float scale, float c2, const float *row_w) {
  const dim3 threads(kRowsThreads);
#define TC_ROWS_SCATTER(MODE, PEN)                                                                                      \
  hipLaunchKernelGGL((rows_scatter_kernel<E, VEC, MODE, PEN>), blocks, threads, 0, stream, in, in_stride, out, osb, ost, y, \
                     ysb, yst, B, rows, cols, scale, c2, row_w)
  if (mode == kCopy)
    TC_ROWS_SCATTER(kCopy, false);
  else if (mode == kScale && !pen)
    TC_ROWS_SCATTER(kScale, false);
  else if (mode == kScale)
    TC_ROWS_SCATTER(kScale, true);
  else if (!pen)
    TC_ROWS_SCATTER(kWeigh, false);
  else
    TC_ROWS_SCATTER(kWeigh, true);
#undef TC_ROWS_SCATTER
}

template <typename E>
int launch_rows_scatter_e(const float *in, int64_t in_stride, void *out_v, int64_t osb, int64_t ost, const void *y_v,
                          int64_t ysb, int64_t yst, int B, int T, int cols, int mode, float scale, float c2,
                          const float *row_w, hipStream_t stream) {
  using bits = typename Elem<E>::bits;
  constexpr int kN = Lane<E>::kN;
  bits *out = static_cast<bits *>(out_v);
  const bits *y = static_cast<const bits *>(y_v);
  const bool pen = y != nullptr;
  const int64_t rows = (int64_t)B * T;
  const dim3 blocks(rows_blocks(rows));
  const bool vec = cols % kN == 0 && (B == 1 || osb % kN == 0) && (T == 1 || ost % kN == 0) && in_stride % 4 == 0 &&
                   aligned(in, 16) && aligned(out_v, 16) &&
                   (!pen || ((B == 1 || ysb % kN == 0) && (T == 1 || yst % kN == 0) && aligned(y_v, 16)));
  if (vec)
    launch_rows_scatter_v<E, true>(mode, pen, blocks, stream, in, in_stride, out, osb, ost, y, ysb, yst, B, rows, cols, scale, c2, row_w);
  else
    launch_rows_scatter_v<E, false>(mode, pen, blocks, stream, in, in_stride, out, osb, ost, y, ysb, yst, B, rows, cols, scale, c2, row_w);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

bool channel_last_strides_ok(int B, int T, int cols, int64_t sb, int64_t st) {
  if (B <= 0 || T <= 0 || cols <= 0) return false;
  if ((B > 1 && sb < cols) || (T > 1 && st < cols)) return false;  // (negative and zero strides, rows that overlap in a row)
  if (B == 1 || T == 1) return true;
  // rows of one dimension nest inside a step of the other: batch-major (b, t) or time-major (t, b)
  const int64_t lim = INT64_MAX / 4;
  if (sb > lim / T || st > lim / B) return false;  // (the products below, and every element offset, fit 63 bits)
  return sb >= (int64_t)(T - 1) * st + cols || st >= (int64_t)(B - 1) * sb + cols;
}

int launch_rows_gather(int dtype, const void *x, int64_t sb, int64_t st, float *out, int64_t out_stride, int B, int T, int cols,
                       hipStream_t stream) {
  if (!x || !out || out_stride < cols || !channel_last_strides_ok(B, T, cols, sb, st)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntLayout);
  switch (dtype) {
    case TC_DTYPE_F32: return launch_rows_gather_e<float>(x, sb, st, out, out_stride, B, T, cols, stream);
    case TC_DTYPE_BF16: return launch_rows_gather_e<__hip_bfloat16>(x, sb, st, out, out_stride, B, T, cols, stream);
    case TC_DTYPE_F16: return launch_rows_gather_e<__half>(x, sb, st, out, out_stride, B, T, cols, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_rows_scatter(int dtype, const float *in, int64_t in_stride, void *out, int64_t osb, int64_t ost, const void *y,
                        int64_t ysb, int64_t yst, int B, int T, int cols, bool scaled, float scale, float pen_c2,
                        const float *row_w, hipStream_t stream) {
  if (!in || !out || in_stride < cols || !channel_last_strides_ok(B, T, cols, osb, ost)) return TC_ERR_INVALID_ARGUMENT;
  const bool pen = pen_c2 > 0.0f;
  if (pen && (!y || !scaled || !channel_last_strides_ok(B, T, cols, ysb, yst))) return TC_ERR_INVALID_ARGUMENT;
  if (!scaled && row_w) return TC_ERR_INVALID_ARGUMENT;
  const int mode = !scaled ? kCopy : (row_w ? kWeigh : kScale);
  const void *yp = pen ? y : nullptr;
  count_launch(kCntLayout);
  switch (dtype) {
    case TC_DTYPE_F32:
      return launch_rows_scatter_e<float>(in, in_stride, out, osb, ost, yp, ysb, yst, B, T, cols, mode, scale, pen_c2, row_w, stream);
    case TC_DTYPE_BF16:
      return launch_rows_scatter_e<__hip_bfloat16>(in, in_stride, out, osb, ost, yp, ysb, yst, B, T, cols, mode, scale, pen_c2, row_w, stream);
    case TC_DTYPE_F16:
      return launch_rows_scatter_e<__half>(in, in_stride, out, osb, ost, yp, ysb, yst, B, T, cols, mode, scale, pen_c2, row_w, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

}  // namespace tc
