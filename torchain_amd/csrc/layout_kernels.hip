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
// The copy back, the rounding copy and the in-place row pass are three of the passes that write a gradient last: each forms
// its elements with half_io.h's last_elem and takes row weights (W) and the out-of-range penalty (PEN) as template flags.
#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kTileC = 64, kTileTMax = 240, kLayoutThreads = 512;
constexpr int kCastThreads = 256, kCastBlocksMax = 4096;

// the (B, C, T) side holds E (the caller's tensor), the 2-D side float32 (the step's scratch)
template <bool TO2D, typename E>
struct LayoutIo {
  using in_t = typename std::conditional<TO2D, typename Elem<E>::bits, float>::type;
  using out_t = typename std::conditional<TO2D, float, typename Elem<E>::bits>::type;
};

// TO2D: in (B, C, T) contiguous -> out[(t*B + b) * out_stride + c];  !TO2D: the inverse, each element as last_elem
// sends it out (E = float: the float32 kernels; otherwise TO2D widens each element it reads, !TO2D rounds each one it
// writes; the tile in LDS stays float32).
// W (!TO2D; tc_chain_step_weighted): out = (scale * row_w[t*B + b]) * in: the factor is loaded once per 2-D row a thread
// reads and folded in as the tile is filled, so the tile holds final float32 values.
// PEN (!TO2D; tc_chain_step_penalized): out = row_w[t*B + b] * penalize(scale * in, y, c2), y the element of pen.y, the
// caller's (B, C, T) network output, at the output's own index.  The penalty precedes the weight, so the tile holds the
// plain values, the factors of the tile's frames follow it in LDS (W), and the write side reads y with the width of its
// stores.
// TC_BCT_AT: where element (c, t) of the block's tile lies in the (B, C, T) tensor, and in pen.y.  An expression spelled
// into each address it forms, not a function: the plain instantiations keep the instruction text they have had.
#define TC_BCT_AT(c, t) (((int64_t)b * Cn + c0 + c) * T + t0 + t)
template <bool TO2D, bool VEC, typename E = float, bool W = false, bool PEN = false>
__global__ __launch_bounds__(kLayoutThreads) void layout_kernel(const typename LayoutIo<TO2D, E>::in_t *__restrict__ in,
                                                                typename LayoutIo<TO2D, E>::out_t *__restrict__ out,
                                                                int B, int Cn, int T, int64_t stride2d, float scale,
                                                                PenArgs<PEN, typename Elem<E>::bits> pen,
                                                                const float *__restrict__ row_w) {
  constexpr bool kF32 = std::is_same<E, float>::value;
  static_assert(!((W || PEN) && TO2D), "row factors and the penalty are for the way back");
  // what happens to an element as the tile is filled, and as it is written
  constexpr int kFill = W && !PEN ? kWeigh : kCopy;
  constexpr int kOut = PEN ? (W ? kWeigh : kScale) : (W ? kCopy : kScale);
  extern __shared__ float tile[];  // kTileC x (frames of the tile | 1), then the frames' factors (W && PEN): sized by
                                   // the launch, several blocks per CU
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
        const uint32_t v = *reinterpret_cast<const uint32_t *>(in + TC_BCT_AT(c, t));
        tile[c * pitch + t] = Elem<E>::widen((uint16_t)(v & 0xFFFFu));
        tile[c * pitch + t + 1] = Elem<E>::widen((uint16_t)(v >> 16));
      }
    } else {
      for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
        const int c = idx / tc, t = idx - c * tc;
        tile[c * pitch + t] = Elem<E>::widen(in[TC_BCT_AT(c, t)]);
      }
    }
    __syncthreads();
    const int cx = tid & (kTileC - 1);
    for (int t = tid / kTileC; t < tc; t += kLayoutThreads / kTileC)
      if (cx < nc) out[((int64_t)(t0 + t) * B + b) * stride2d + c0 + cx] = tile[cx * pitch + t];
  } else {
    float *wt = tile + kTileC * pitch;
    auto fill = [&](float v, float w) -> float { return last_elem<kFill, false, true>(v, 0.0f, w, scale, 0.0f); };
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
        if constexpr (kFill != kCopy) {
          const float w = row_w[(int64_t)(t0 + t) * B + b];
          v = make_float4(fill(v.x, w), fill(v.y, w), fill(v.z, w), fill(v.w, w));
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
          tile[cx * pitch + t] = kFill != kCopy ? fill(v, row_w[(int64_t)(t0 + t) * B + b]) : v;
        }
    }
    if constexpr (W && PEN)
      for (int t = tid; t < tc; t += kLayoutThreads) wt[t] = row_w[(int64_t)(t0 + t) * B + b];
    __syncthreads();
    // an element v of frame t of the tile as it leaves, y its network output
    auto fin = [&](float v, int t, float y) -> float {
      const float w = W && PEN ? wt[t] : 1.0f;
      // (F32 for every E: without the penalty this kernel has always left a 16-bit element's one product to the backend,
      // as a float32 one's -- on the element-wise float16 path it is fused into the conversion.  On record, and kept.)
      return last_elem<kOut, PEN, true>(v, y, w, scale, pen.c2);
    };
    if constexpr (!kF32) {
      // frames t and t + 1 of channel c, rounded once and packed; yv: the dword that holds their two network outputs
      auto fin2 = [&](const float *src, int t, uint32_t yv) -> uint32_t {
        return Elem<E>::round(fin(src[0], t, Elem<E>::widen((uint16_t)(yv & 0xFFFFu)))) |
               ((uint32_t)Elem<E>::round(fin(src[1], t + 1, Elem<E>::widen((uint16_t)(yv >> 16)))) << 16);
      };
      // Write side of a 16-bit tensor: 8-byte stores (4 frames) when every run starts 8-byte aligned, 4-byte ones
      // (2 frames) when it starts 4-byte aligned
      if (VEC && (T & 3) == 0) {
        const int quad = tc / 4;
        for (int idx = tid; idx < nc * quad; idx += kLayoutThreads) {
          const int c = idx / quad, t = 4 * (idx - c * quad);
          const float *src = tile + c * pitch + t;
          uint2 yv = make_uint2(0u, 0u);
          if constexpr (PEN) yv = *reinterpret_cast<const uint2 *>(pen.y + TC_BCT_AT(c, t));
          *reinterpret_cast<uint2 *>(out + TC_BCT_AT(c, t)) = make_uint2(fin2(src, t, yv.x), fin2(src + 2, t + 2, yv.y));
        }
      } else if (VEC && (T & 1) == 0) {
        const int half = tc / 2;
        for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
          const int c = idx / half, t = 2 * (idx - c * half);
          const float *src = tile + c * pitch + t;
          uint32_t yv = 0u;
          if constexpr (PEN) yv = *reinterpret_cast<const uint32_t *>(pen.y + TC_BCT_AT(c, t));
          *reinterpret_cast<uint32_t *>(out + TC_BCT_AT(c, t)) = fin2(src, t, yv);
        }
      } else {
        for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
          const int c = idx / tc, t = idx - c * tc;
          uint16_t yv = 0;
          if constexpr (PEN) yv = pen.y[TC_BCT_AT(c, t)];
          out[TC_BCT_AT(c, t)] = Elem<E>::round(fin(tile[c * pitch + t], t, Elem<E>::widen(yv)));
        }
      }
    } else {
      // Write side: runs of tc floats per channel; 8-byte stores when every run starts 8-byte aligned
      if (VEC && (T & 1) == 0 && (tc & 1) == 0) {
        const int half = tc / 2;
        for (int idx = tid; idx < nc * half; idx += kLayoutThreads) {
          const int c = idx / half, t = 2 * (idx - c * half);
          float2 yv = make_float2(0.f, 0.f);
          if constexpr (PEN) yv = *reinterpret_cast<const float2 *>(pen.y + TC_BCT_AT(c, t));
          *reinterpret_cast<float2 *>(out + TC_BCT_AT(c, t)) = make_float2(fin(tile[c * pitch + t], t, yv.x), fin(tile[c * pitch + t + 1], t + 1, yv.y));
        }
      } else {
        for (int idx = tid; idx < nc * tc; idx += kLayoutThreads) {
          const int c = idx / tc, t = idx - c * tc;
          float yv = 0.f;
          if constexpr (PEN) yv = pen.y[TC_BCT_AT(c, t)];
          out[TC_BCT_AT(c, t)] = fin(tile[c * pitch + t], t, yv);
        }
      }
    }
  }
}
#undef TC_BCT_AT

// 16-bit 2-D input -> float32: (rows, cols) with `in_stride` -> contiguous (rows, cols), one wave per row at a time.
// VEC: 16-byte loads (8 elements) and two 16-byte stores, when cols and in_stride are multiples of 8 and both bases
// 16-byte aligned.
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
// (n a multiple of 8, all bases 16-byte aligned; with W, cols a multiple of 8 too).  W (tc_chain_step_weighted): element i
// is row i / cols of a (rows, cols) matrix and is rounded from row_w[row] * in[i].  PEN: from row_w[row] * penalize(in[i],
// pen.y[i], c2), pen.y the widened network output, n contiguous floats as well.
template <typename E, bool VEC, bool W = false, bool PEN = false>
__global__ __launch_bounds__(kCastThreads) void round_kernel(const float *__restrict__ in, uint16_t *__restrict__ out,
                                                             int64_t n, const float *__restrict__ row_w, int cols,
                                                             PenArgs<PEN, float> pen) {
  constexpr int kMode = W ? kWeigh : (PEN ? kScale : kCopy);
  auto fin = [&](float v, float y, float f) -> float { return last_elem<kMode, PEN, false>(v, y, f, 1.0f, pen.c2); };
  const int64_t step = (int64_t)gridDim.x * kCastThreads;
  if (VEC) {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n / 8; i += step) {
      float4 a = reinterpret_cast<const float4 *>(in)[2 * i], b = reinterpret_cast<const float4 *>(in)[2 * i + 1];
      float4 ya = make_float4(0.f, 0.f, 0.f, 0.f), yb = ya;
      if constexpr (PEN) ya = reinterpret_cast<const float4 *>(pen.y)[2 * i], yb = reinterpret_cast<const float4 *>(pen.y)[2 * i + 1];
      if constexpr (kMode != kCopy) {
        const float f = W ? row_w[8 * i / cols] : 1.0f;  // (the 8 elements lie in one row)
        a = make_float4(fin(a.x, ya.x, f), fin(a.y, ya.y, f), fin(a.z, ya.z, f), fin(a.w, ya.w, f));
        b = make_float4(fin(b.x, yb.x, f), fin(b.y, yb.y, f), fin(b.z, yb.z, f), fin(b.w, yb.w, f));
      }
      auto pack = [](float lo, float hi) { return (uint32_t)Elem<E>::round(lo) | ((uint32_t)Elem<E>::round(hi) << 16); };
      reinterpret_cast<uint4 *>(out)[i] = make_uint4(pack(a.x, a.y), pack(a.z, a.w), pack(b.x, b.y), pack(b.z, b.w));
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kCastThreads + threadIdx.x; i < n; i += step) {
      const float f = W ? row_w[i / cols] : 1.0f;
      out[i] = Elem<E>::round(fin(in[i], PEN ? pen.y[i] : 0.0f, f));
    }
  }
}

// a[r][c] = row_w[r] * a[r][c] in place, contiguous float32 (rows, cols), one wave per row at a time (the factor is
// loaded once per row and wave).  PEN: a[r][c] = row_w[r] * penalize(a[r][c], pen.y[r * pen.stride + c], c2) (W false: no
// row factor), pen.y the caller's own 2-D network output.  VEC: 16-byte loads and stores (cols, and pen.stride, multiples
// of 4, bases 16-byte aligned).
template <bool VEC, bool W, bool PEN>
__global__ __launch_bounds__(kCastThreads) void scale_rows_kernel(float *__restrict__ a, int64_t rows, int cols,
                                                                  PenArgs<PEN, float> pen, const float *__restrict__ row_w) {
  static_assert(W || PEN, "a pass that changes nothing");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * (kCastThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kCastThreads / 64)) {
    const float f = W ? row_w[r] : 1.0f;
    float *row = a + r * cols;
    const float *yr = PEN ? pen.y + r * pen.stride : nullptr;
    auto fin = [&](float v, float y) -> float { return last_elem<W ? kWeigh : kScale, PEN, true>(v, y, f, 1.0f, pen.c2); };
    if (VEC) {
      for (int c = lane * 4; c < cols; c += 64 * 4) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c);
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (PEN) u = *reinterpret_cast<const float4 *>(yr + c);
        *reinterpret_cast<float4 *>(row + c) = make_float4(fin(v.x, u.x), fin(v.y, u.y), fin(v.z, u.z), fin(v.w, u.w));
      }
    } else {
      for (int c = lane; c < cols; c += 64) row[c] = fin(row[c], PEN ? yr[c] : 0.0f);
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

int cast_blocks(int64_t items) {
  const int64_t b = (items + kCastThreads - 1) / kCastThreads;
  return (int)(b < 1 ? 1 : b > kCastBlocksMax ? kCastBlocksMax : b);
}

// the tiled copy, either way, with the (B, C, T) side of E
template <typename E>
int launch_tiled(bool to2d, const void *in_v, void *out_v, int B, int Cn, int T, int64_t stride2d, const LastPass &lp,
                 hipStream_t stream) {
  using bits = typename Elem<E>::bits;
  constexpr bool kF32 = std::is_same<E, float>::value;
  const bool pen = lp.pen_c2 > 0.0f, w = lp.row_w != nullptr;
  if (!in_v || !out_v || B <= 0 || Cn <= 0 || T <= 0 || stride2d < Cn) return TC_ERR_INVALID_ARGUMENT;
  if ((to2d && (w || pen)) || (pen && !lp.y)) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_grid_ok(B, T)) return TC_ERR_UNSUPPORTED;
  count_launch(kCntLayout);
  const dim3 grid((Cn + kTileC - 1) / kTileC, B, (T + kTileTMax - 1) / kTileTMax), threads(kLayoutThreads);
  const size_t frames = (size_t)(T < kTileTMax ? T : kTileTMax);
  const size_t lds = sizeof(float) * (kTileC * (frames | 1) + (w && pen ? frames : 0));
  if (to2d) {
    // (16-bit: dword loads of two frames; float32 has the one form)
    const bool vec = !kF32 && (T & 1) == 0 && aligned(in_v, 4);
    with_bools(
        [&](auto v) {
          constexpr bool kVec = decltype(v)::value;
          if constexpr (!(kF32 && kVec))
            hipLaunchKernelGGL((layout_kernel<true, kVec, E>), grid, threads, lds, stream, static_cast<const bits *>(in_v),
                               static_cast<float *>(out_v), B, Cn, T, stride2d, lp.scale, PenArgs<false, bits>{}, nullptr);
        },
        vec);
  } else {
    // 16-byte path of the 2-D side: rows and base 16-byte aligned, whole float4s of channels in every tile; 8-byte
    // accesses of the (B, C, T) side, y travelling with the output
    const bool vec = stride2d % 4 == 0 && aligned(in_v, 16) && aligned(out_v, 8) && (!pen || aligned(lp.y, 8));
    with_bools(
        [&](auto v, auto wt, auto p) {
          constexpr bool kPen = decltype(p)::value;
          PenArgs<kPen, bits> pa;
          if constexpr (kPen) pa = {static_cast<const bits *>(lp.y), 0, lp.pen_c2};
          hipLaunchKernelGGL((layout_kernel<false, decltype(v)::value, E, decltype(wt)::value, kPen>), grid, threads, lds, stream,
                             static_cast<const float *>(in_v), static_cast<bits *>(out_v), B, Cn, T, stride2d, lp.scale,
                             pa, lp.row_w);
        },
        vec, w, pen);
  }
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

bool layout_grid_ok(int B, int T) { return B <= 65535 && (T + kTileTMax - 1) / kTileTMax <= 65535; }  // grid y / z limits

int launch_to2d(int dtype, const void *in_bct, float *out, int B, int Cn, int T, int64_t stride2d, hipStream_t stream) {
  return with_elem(dtype, [&](auto e) {
    return launch_tiled<typename decltype(e)::type>(true, in_bct, out, B, Cn, T, stride2d, LastPass{}, stream);
  });
}

int launch_from2d(int dtype, const float *in, int64_t stride2d, void *out_bct, int B, int Cn, int T, const LastPass &lp,
                  hipStream_t stream) {
  return with_elem(dtype, [&](auto e) {
    return launch_tiled<typename decltype(e)::type>(false, in, out_bct, B, Cn, T, stride2d, lp, stream);
  });
}

int launch_widen_rows(int dtype, const void *in, int64_t in_stride, float *out, int64_t rows, int cols, hipStream_t stream) {
  const int blocks = cast_blocks(rows * 64);  // (a wave per row)
  const bool vec = cols % 8 == 0 && in_stride % 8 == 0 && aligned(in, 16) && aligned(out, 16);
  const int rc = with_elem<false>(dtype, [&](auto e) {
    with_bools(
        [&](auto v) {
          hipLaunchKernelGGL((widen_rows_kernel<typename decltype(e)::type, decltype(v)::value>), dim3(blocks), dim3(kCastThreads),
                             0, stream, static_cast<const uint16_t *>(in), in_stride, out, rows, cols);
        },
        vec);
    return TC_OK;
  });
  if (rc != TC_OK) return rc;
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_round(int dtype, const float *in, void *out, int64_t n, int cols, const LastPass &lp, hipStream_t stream) {
  const bool pen = lp.pen_c2 > 0.0f, w = lp.row_w != nullptr;
  const float *y = static_cast<const float *>(lp.y);
  if (!in || !out || n <= 0 || lp.scale != 1.0f || (pen && !y) || (w && cols <= 0)) return TC_ERR_INVALID_ARGUMENT;
  const bool vec = n % 8 == 0 && aligned(in, 16) && aligned(out, 16) && (!pen || aligned(y, 16)) && (!w || cols % 8 == 0);
  const dim3 blocks(cast_blocks(vec ? n / 8 : n)), threads(kCastThreads);
  const int rc = with_elem<false>(dtype, [&](auto e) {
    with_bools(
        [&](auto v, auto wt, auto p) {
          constexpr bool kPen = decltype(p)::value;
          PenArgs<kPen, float> pa;
          if constexpr (kPen) pa = {y, 0, lp.pen_c2};
          hipLaunchKernelGGL((round_kernel<typename decltype(e)::type, decltype(v)::value, decltype(wt)::value, kPen>), blocks,
                             threads, 0, stream, in, static_cast<uint16_t *>(out), n, lp.row_w, cols, pa);
        },
        vec, w, pen);
    return TC_OK;
  });
  if (rc != TC_OK) return rc;
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_scale_rows(float *a, int64_t rows, int cols, const LastPass &lp, hipStream_t stream) {
  const bool pen = lp.pen_c2 > 0.0f, w = lp.row_w != nullptr;
  const float *y = static_cast<const float *>(lp.y);
  if (!a || rows <= 0 || cols <= 0 || lp.scale != 1.0f || !(w || pen) || (pen && (!y || lp.y_stride < cols)))
    return TC_ERR_INVALID_ARGUMENT;
  const dim3 blocks(cast_blocks(rows * 64)), threads(kCastThreads);  // (a wave per row)
  const bool vec = cols % 4 == 0 && aligned(a, 16) && (!pen || (lp.y_stride % 4 == 0 && aligned(y, 16)));
  with_bools(
      [&](auto v, auto wt, auto p) {
        constexpr bool kW = decltype(wt)::value, kPen = decltype(p)::value;
        PenArgs<kPen, float> pa;
        if constexpr (kPen) pa = {y, lp.y_stride, lp.pen_c2};
        if constexpr (kW || kPen)
          hipLaunchKernelGGL((scale_rows_kernel<decltype(v)::value, kW, kPen>), blocks, threads, 0, stream, a, rows, cols, pa, lp.row_w);
      },
      vec, w, pen);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
