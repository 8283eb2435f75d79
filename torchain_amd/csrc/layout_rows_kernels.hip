// Channel-last views at the library's edge (tc_chain_step_strided, TC_LAYOUT_CHANNEL_LAST): a (B, C, T) tensor whose channel
// stride is 1 -- the output of a batch-first LSTM or Transformer passed as out.transpose(1, 2), or one half of a joint head --
// has its element (b, c, t) at b*sb + t*st + c.  Its rows are whole already, so the way in and the way out are row copies with
// a permuted row index, not transposes: no LDS, one wave per row at a time, 16-byte lanes where every address allows them.
//   gather  : y2d[(t*B + b) * stride + c] = widen(x[b*sb + t*st + c])                      (float32 / bfloat16 / float16 in)
//   scatter : out[b*osb + t*ost + c] = round(f(in2d[(t*B + b) * stride + c]))              (float32 in)
// with f the element function of every last pass (half_io.h: last_elem), the one the (B, C, T) copy back calls -- plain
// scale * v; with row weights (scale * w[row]) * v; with the penalty w[row] * penalize(scale * v, y) -- so that a channel-last
// step returns the bits of the step on the contiguous copy.
#include <algorithm>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kRowsThreads = 256, kRowsBlocksMax = 4096;

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

// in[(t*B + b) * in_stride + c] (float32) -> out[b*osb + t*ost + c] (E), each element as last_elem<MODE, PEN> sends it out,
// rounded once.  PEN: y = widen(yx[b*ysb + t*yst + c]), the network output at the index the element is written to.
// VEC: cols, osb, ost (PEN: ysb, yst too) multiples of Lane<E>::kN, in_stride a multiple of 4, all bases 16-byte aligned.
template <typename E, bool VEC, int MODE, bool PEN>
__global__ __launch_bounds__(kRowsThreads) void rows_scatter_kernel(const float *__restrict__ in, int64_t in_stride,
                                                                    typename Elem<E>::bits *__restrict__ out, int64_t osb,
                                                                    int64_t ost, const typename Elem<E>::bits *__restrict__ yx,
                                                                    int64_t ysb, int64_t yst, int B, int64_t rows, int cols,
                                                                    float scale, float c2, const float *__restrict__ row_w) {
  constexpr bool kF32 = std::is_same<E, float>::value;
  constexpr int kN = Lane<E>::kN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kRowsThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kRowsThreads / 64)) {
    const int64_t t = r / B, b = r - t * B;
    const float *src = in + r * in_stride;
    typename Elem<E>::bits *dst = out + b * osb + t * ost;
    const typename Elem<E>::bits *yr = PEN ? yx + b * ysb + t * yst : nullptr;
    const float w = MODE == kWeigh ? row_w[r] : 1.0f;
    auto fin = [&](float v, float y) -> float { return last_elem<MODE, PEN, kF32>(v, y, w, scale, c2); };
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
  with_bools(
      [&](auto v) {
        hipLaunchKernelGGL((rows_gather_kernel<E, decltype(v)::value>), blocks, threads, 0, stream, x, sb, st, out, out_stride, B,
                           rows, cols);
      },
      vec);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_rows_scatter_e(const float *in, int64_t in_stride, void *out_v, int64_t osb, int64_t ost, int B, int T, int cols,
                          const LastPass &lp, hipStream_t stream) {
  using bits = typename Elem<E>::bits;
  constexpr int kN = Lane<E>::kN;
  bits *out = static_cast<bits *>(out_v);
  const bool pen = lp.pen_c2 > 0.0f;
  const bits *y = pen ? static_cast<const bits *>(lp.y) : nullptr;
  const int64_t rows = (int64_t)B * T, ysb = lp.y_stride, yst = lp.y_st;
  const dim3 blocks(rows_blocks(rows)), threads(kRowsThreads);
  const bool vec = cols % kN == 0 && (B == 1 || osb % kN == 0) && (T == 1 || ost % kN == 0) && in_stride % 4 == 0 &&
                   aligned(in, 16) && aligned(out_v, 16) &&
                   (!pen || ((B == 1 || ysb % kN == 0) && (T == 1 || yst % kN == 0) && aligned(y, 16)));
  with_bools(
      [&](auto v, auto scaled, auto weighted, auto p) {
        constexpr bool kScaled = decltype(scaled)::value, kW = decltype(weighted)::value, kPen = decltype(p)::value;
        constexpr int kMode = !kScaled ? kCopy : (kW ? kWeigh : kScale);
        if constexpr (kScaled || !(kW || kPen))
          hipLaunchKernelGGL((rows_scatter_kernel<E, decltype(v)::value, kMode, kPen>), blocks, threads, 0, stream, in, in_stride,
                             out, osb, ost, y, ysb, yst, B, rows, cols, lp.scale, lp.pen_c2, lp.row_w);
      },
      vec, lp.scaled, lp.row_w != nullptr, pen);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// Ragged minibatches: +0 into the padding of an output tensor, frames seq_frames[b] .. T - 1 of sequence b.  A block takes
// one sequence's share; consecutive threads take consecutive frames where those are the tensor's unit stride ((B, C, T)),
// else consecutive channels.  A sequence of full length costs its blocks one scalar load.
template <typename Bits>
__global__ __launch_bounds__(kRowsThreads) void zero_padding_kernel(Bits *out, int64_t sb, int64_t st, int64_t sc, int B, int T,
                                                                    int cols, const int32_t *__restrict__ seq_frames) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int first = ragged_frames(seq_frames, b, T), pad = T - first;
    if (pad <= 0) continue;
    const int64_t n = (int64_t)pad * cols;
    Bits *const base = out + (int64_t)b * sb;
    for (int64_t i = (int64_t)blockIdx.x * kRowsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowsThreads) {
      int64_t f, c;
      if (st < sc) {
        c = i / pad;
        f = i - c * pad;
      } else {
        f = i / cols;
        c = i - f * cols;
      }
      base[(first + f) * st + c * sc] = Bits(0);
    }
  }
}

// The isolating step: zero_padding_kernel on the frames that survive, alive_frames[b] in 0 .. T -- 0 for a failed sequence,
// all of whose rows go (ragged_frames holds a length to 1 .. T; a sibling, so that zero_padding_kernel stays as it is).
template <typename Bits>
__global__ __launch_bounds__(kRowsThreads) void zero_failed_kernel(Bits *out, int64_t sb, int64_t st, int64_t sc, int B, int T,
                                                                   int cols, const int32_t *__restrict__ alive_frames) {
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int f0 = __builtin_amdgcn_readfirstlane(alive_frames[b]);
    const int first = f0 < 0 ? 0 : (f0 > T ? T : f0), pad = T - first;
    if (pad <= 0) continue;
    const int64_t n = (int64_t)pad * cols;
    Bits *const base = out + (int64_t)b * sb;
    for (int64_t i = (int64_t)blockIdx.x * kRowsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowsThreads) {
      int64_t f, c;
      if (st < sc) {
        c = i / pad;
        f = i - c * pad;
      } else {
        f = i / cols;
        c = i - f * cols;
      }
      base[(first + f) * st + c * sc] = Bits(0);
    }
  }
}

}  // namespace

int launch_zero_failed(void *out, int elem_bytes, int64_t sb, int64_t st, int64_t sc, int B, int T, int cols,
                       const int32_t *alive_frames, hipStream_t stream) {
  if (!out || !alive_frames || B <= 0 || T <= 0 || cols <= 0 || (elem_bytes != 4 && elem_bytes != 2)) return TC_ERR_INVALID_ARGUMENT;
  const int64_t per_seq = ((int64_t)T * cols + kRowsThreads - 1) / kRowsThreads;
  const dim3 blocks((unsigned)std::min<int64_t>(per_seq, 64), (unsigned)std::min(B, 65535)), threads(kRowsThreads);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(zero_failed_kernel<uint32_t>, blocks, threads, 0, stream, static_cast<uint32_t *>(out), sb, st, sc, B, T, cols, alive_frames);
  else
    hipLaunchKernelGGL(zero_failed_kernel<uint16_t>, blocks, threads, 0, stream, static_cast<uint16_t *>(out), sb, st, sc, B, T, cols, alive_frames);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_zero_padding(void *out, int elem_bytes, int64_t sb, int64_t st, int64_t sc, int B, int T, int cols,
                        const int32_t *seq_frames, hipStream_t stream) {
  if (!out || !seq_frames || B <= 0 || T <= 0 || cols <= 0 || (elem_bytes != 4 && elem_bytes != 2)) return TC_ERR_INVALID_ARGUMENT;
  const int64_t per_seq = ((int64_t)T * cols + kRowsThreads - 1) / kRowsThreads;
  const dim3 blocks((unsigned)std::min<int64_t>(per_seq, 64), (unsigned)std::min(B, 65535)), threads(kRowsThreads);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(zero_padding_kernel<uint32_t>, blocks, threads, 0, stream, static_cast<uint32_t *>(out), sb, st, sc, B, T, cols, seq_frames);
  else
    hipLaunchKernelGGL(zero_padding_kernel<uint16_t>, blocks, threads, 0, stream, static_cast<uint16_t *>(out), sb, st, sc, B, T, cols, seq_frames);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

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
  return with_elem(dtype, [&](auto e) {
    return launch_rows_gather_e<typename decltype(e)::type>(x, sb, st, out, out_stride, B, T, cols, stream);
  });
}

int launch_rows_scatter(int dtype, const float *in, int64_t in_stride, void *out, int64_t osb, int64_t ost, int B, int T,
                        int cols, const LastPass &lp, hipStream_t stream) {
  if (!in || !out || in_stride < cols || !channel_last_strides_ok(B, T, cols, osb, ost)) return TC_ERR_INVALID_ARGUMENT;
  if (lp.pen_c2 > 0.0f && (!lp.y || !lp.scaled || !channel_last_strides_ok(B, T, cols, lp.y_stride, lp.y_st)))
    return TC_ERR_INVALID_ARGUMENT;
  if (!lp.scaled && lp.row_w) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntLayout);
  return with_elem(dtype, [&](auto e) {
    return launch_rows_scatter_e<typename decltype(e)::type>(in, in_stride, out, osb, ost, B, T, cols, lp, stream);
  });
}

}  // namespace tc
