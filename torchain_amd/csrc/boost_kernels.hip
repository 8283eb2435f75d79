// Boosted LF-MMI (tc_chain_step_boosted): every denominator path's weight is multiplied by exp(-b * A(path)),
// A the path's frame accuracy against a reference.  Frame accuracy is additive over frames, so the boost is a shift of the
// denominator's input alone,
//     y_b[t*S + s, j] = fl32(y32 - fl32(b32 * a_t(j))),
// two float32 roundings (__fmul_rn, __fsub_rn: never one FMA), with a_t(j) the accuracy of tc_den_expected_accuracy: the
// indicator of (ref_dev, class_dev), or a dense float32 matrix.  The numerator, the l2 term, the penalty and the row weights
// keep the true y.
//   boost pass : the denominator's private frame-major float32 matrix, formed from the caller's tensor where it lies -- rows
//                with unit channel stride at s*sb + t*st (2-D rows: sb = row_stride, st = S * row_stride; channel-last views),
//                one wave per row, 16-byte accesses where every address allows them and scalar tails; or a contiguous
//                (B, C, T) tensor, tiled through LDS as the plain copy is.  It stands in for launch_to2d / launch_rows_gather /
//                launch_widen_rows on the denominator's side: one pass, reads y and (dense) a, writes y_b.
//   l2 fix-up  : the denominator kernels fold -l2_scale * y' and sum(y'^2) of the matrix they read into their own passes.
//                With d = fl32(b32 * a), y = y_b + d up to the one rounding of y_b, so
//                    sum(y^2)  = sum(y_b^2) + sum(2 * y_b * d + d^2)      (doubles, a fixed order per sequence)
//                    -l2 * y   = -l2 * y_b - l2 * d
//                over the elements with d != 0 only: S * T of them for a hard reference without classes.  Two small launches,
//                and none when l2 == 0.
// Rows of frames t >= T_s of a ragged batch: neither the reference nor the accuracy row is read; y_b is the widened y there.
#include <algorithm>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kBoostThreads = 256, kBoostBlocksMax = 4096;
constexpr int kBoostTileC = 64, kBoostTileTMax = 240, kBoostTileThreads = 512;
constexpr int kFixThreads = 1024;

template <typename E>
struct BoostLane {
  static constexpr int kN = std::is_same<E, float>::value ? 4 : 8;
};

// y - b * a in two roundings.  __fmul_rn is a plain product to the backend, which contracts it into the difference under
// the build's default -ffp-contract; the empty asm keeps the product a float32 value of its own (as half_io.h's weigh).
__device__ __forceinline__ float boosted(float y, float b, float a) {
  float p = __fmul_rn(b, a);
  asm volatile("" : "+v"(p));
  return __fsub_rn(y, p);
}

// the sequence's own frames, held to 1 .. T (device memory no host code has seen)
__device__ __forceinline__ int own_frames(const int32_t *seq_frames, int s, int T) {
  if (!seq_frames) return T;
  const int f = seq_frames[s];
  return f < 1 ? 1 : (f > T ? T : f);
}

// The hard reference of frame (s, t): whether the frame scores at all, and the reference pdf's class (without classes the
// pdf itself, the one pdf that scores).
struct HardRef {
  bool scores;
  int32_t cls;
};
__device__ __forceinline__ HardRef hard_ref(const BoostAcc &a, int s, int t, int T, int P) {
  HardRef h;
  const int32_t rv = a.ref[(int64_t)s * T + t];
  h.scores = rv >= 0 && rv < P;
  h.cls = h.scores ? (a.cls ? a.cls[rv] : rv) : 0;
  return h;
}
__device__ __forceinline__ float hard_acc(const BoostAcc &a, const HardRef &h, int c) {
  return h.scores && (a.cls ? a.cls[c] : c) == h.cls ? 1.0f : 0.0f;
}

template <typename E>
__device__ __forceinline__ void load_elems(const typename Elem<E>::bits *p, float (&v)[BoostLane<E>::kN]) {
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

// x[s*sb + t*st + c] (E) -> out[(t*S + s) * out_stride + c] (float32), rows = T * S, a wave per row at a time.
// VEC: sb, st multiples of the lane's elements, out_stride (DENSE: the accuracy's row stride too) a multiple of 4, every base
// 16-byte aligned; the columns beyond the last whole lane are a scalar tail.  DENSE: a is the accuracy matrix's row.
template <typename E, bool VEC, bool DENSE>
__global__ __launch_bounds__(kBoostThreads) void boost_rows_kernel(const typename Elem<E>::bits *__restrict__ x, int64_t sb,
                                                                  int64_t st, float *__restrict__ out, int64_t out_stride,
                                                                  int S, int T, int cols, BoostAcc a) {
  constexpr int kN = BoostLane<E>::kN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = (int64_t)S * T;
  for (int64_t r = (int64_t)blockIdx.x * (kBoostThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kBoostThreads / 64)) {
    const int64_t t = r / S;
    const int s = (int)(r - t * S);
    const typename Elem<E>::bits *src = x + (int64_t)s * sb + t * st;
    float *dst = out + r * out_stride;
    const bool live = (int)t < own_frames(a.seq_frames, s, T);
    const float *arow = DENSE && live ? a.acc + r * a.acc_stride : nullptr;
    HardRef h;
    h.scores = false;
    h.cls = 0;
    if (!DENSE && live) h = hard_ref(a, s, (int)t, T, cols);
    auto at = [&](int c) -> float { return DENSE ? (live ? arow[c] : 0.0f) : hard_acc(a, h, c); };
    int c_tail = 0;
    if (VEC) {
      c_tail = cols - cols % kN;
      for (int c = lane * kN; c < c_tail; c += 64 * kN) {
        float v[kN], av[kN];
        load_elems<E>(src + c, v);
        if (DENSE && live) {
#pragma unroll
          for (int i = 0; i < kN; i += 4) {
            const float4 q = *reinterpret_cast<const float4 *>(arow + c + i);
            av[i] = q.x, av[i + 1] = q.y, av[i + 2] = q.z, av[i + 3] = q.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < kN; ++i) av[i] = at(c + i);
        }
#pragma unroll
        for (int i = 0; i < kN; ++i) v[i] = live ? boosted(v[i], a.b, av[i]) : v[i];
#pragma unroll
        for (int i = 0; i < kN; i += 4) *reinterpret_cast<float4 *>(dst + c + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
      }
    }
    for (int c = c_tail + lane; c < cols; c += 64) {
      const float y = Elem<E>::widen(src[c]);
      dst[c] = live ? boosted(y, a.b, at(c)) : y;
    }
  }
}

// in (B, C, T) contiguous (E) -> out[(t*B + b) * out_stride + c] (float32): a [64 channels] x [<= 240 frames] tile of one
// sequence through LDS, read in runs along t and written in runs along c, the boost applied on the way out.
template <typename E, bool DENSE>
__global__ __launch_bounds__(kBoostTileThreads) void boost_bct_kernel(const typename Elem<E>::bits *__restrict__ in,
                                                                     float *__restrict__ out, int64_t out_stride, int B, int Cn,
                                                                     int T, BoostAcc a) {
  extern __shared__ float boost_tile[];
  const int c0 = blockIdx.x * kBoostTileC, b = blockIdx.y, t0 = blockIdx.z * kBoostTileTMax;
  const int tc = min(kBoostTileTMax, T - t0), nc = min(kBoostTileC, Cn - c0);
  const int pitch = tc | 1;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < nc * tc; idx += kBoostTileThreads) {
    const int c = idx / tc, t = idx - c * tc;
    boost_tile[c * pitch + t] = Elem<E>::widen(in[((int64_t)b * Cn + c0 + c) * T + t0 + t]);
  }
  __syncthreads();
  const int own = own_frames(a.seq_frames, b, T);
  const int cx = tid & (kBoostTileC - 1);
  for (int t = tid / kBoostTileC; t < tc; t += kBoostTileThreads / kBoostTileC) {
    if (cx >= nc) continue;
    const int64_t r = (int64_t)(t0 + t) * B + b;
    const float y = boost_tile[cx * pitch + t];
    float v = y;
    if (t0 + t < own) {
      float av;
      if (DENSE) {
        av = a.acc[r * a.acc_stride + c0 + cx];
      } else {
        const HardRef h = hard_ref(a, b, t0 + t, T, Cn);
        av = hard_acc(a, h, c0 + cx);
      }
      v = boosted(y, a.b, av);
    }
    out[r * out_stride + c0 + cx] = v;
  }
}

// sum over the sequence's live frames of 2 * y_b * d + d^2, d = fl32(b * a), over the elements with d != 0: added to
// seq_y2[s], which the denominator left as sum(y_b^2).  One workgroup per sequence, a fixed order: thread i takes elements i,
// i + 1024, ... of the sequence's frames (hard reference without classes), or wave w takes frames w, w + 16, ... and a lane
// its columns in order (VEC: four at a time, 16-byte loads of a and y_b -- P, both strides multiples of 4, both bases 16-byte
// aligned); thread 0 adds the partials.
template <bool DENSE, bool VEC>
__global__ __launch_bounds__(kFixThreads) void boost_l2_sum_kernel(const float *__restrict__ yb, int64_t yb_stride, int S, int T,
                                                                  int P, BoostAcc a, double *__restrict__ seq_y2) {
  __shared__ double part[kFixThreads];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int own = own_frames(a.seq_frames, s, T);
  double acc = 0.0;
  auto add = [&](float v, float av) {
    const float d = __fmul_rn(a.b, av);
    const double dd = (double)d;
    // (d != 0 holds for a NaN too: the sequence's sum is non-finite with it, as the denominator's own already is)
    acc += d != 0.0f ? 2.0 * (double)v * dd + dd * dd : 0.0;
  };
  if (!DENSE && !a.cls) {
    for (int t = tid; t < own; t += kFixThreads) {
      const HardRef h = hard_ref(a, s, t, T, P);
      if (h.scores) add(yb[((int64_t)t * S + s) * yb_stride + h.cls], 1.0f);
    }
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    for (int t = wave; t < own; t += kFixThreads / 64) {
      const int64_t r = (int64_t)t * S + s;
      const float *yr = yb + r * yb_stride;
      if (DENSE) {
        const float *arow = a.acc + r * a.acc_stride;
        if (VEC) {
          for (int c = lane * 4; c < P; c += 256) {
            const float4 av = *reinterpret_cast<const float4 *>(arow + c), yv = *reinterpret_cast<const float4 *>(yr + c);
            add(yv.x, av.x), add(yv.y, av.y), add(yv.z, av.z), add(yv.w, av.w);
          }
        } else {
          for (int c = lane; c < P; c += 64) add(yr[c], arow[c]);
        }
      } else {
        const HardRef h = hard_ref(a, s, t, T, P);
        if (!h.scores) continue;
        for (int c = lane; c < P; c += 64)
          if (a.cls[c] == h.cls) add(yr[c], 1.0f);
      }
    }
  }
  part[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < kFixThreads; ++i) sum += part[i];
    seq_y2[s] += sum;
  }
}

// g[r, c] -= l2_scale * d over the live rows' elements with d != 0: the denominator wrote -l2_scale * y_b, the caller is owed
// -l2_scale * y.  A wave per row at a time.  VEC (the dense form): 16-byte accesses of a and g -- P, both strides multiples
// of 4, both bases 16-byte aligned.
template <bool DENSE, bool VEC>
__global__ __launch_bounds__(kBoostThreads) void boost_l2_grad_kernel(float *__restrict__ g, int64_t g_stride, int S, int T, int P,
                                                                     BoostAcc a, float l2_scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = (int64_t)S * T;
  for (int64_t r = (int64_t)blockIdx.x * (kBoostThreads / 64) + wave; r < rows; r += (int64_t)gridDim.x * (kBoostThreads / 64)) {
    const int64_t t = r / S;
    const int s = (int)(r - t * S);
    if ((int)t >= own_frames(a.seq_frames, s, T)) continue;
    float *row = g + r * g_stride;
    if (DENSE) {
      const float *arow = a.acc + r * a.acc_stride;
      auto fix = [&](float gv, float av) -> float {
        const float d = __fmul_rn(a.b, av);
        return d != 0.0f ? gv - l2_scale * d : gv;
      };
      if (VEC) {
        for (int c = lane * 4; c < P; c += 256) {
          const float4 av = *reinterpret_cast<const float4 *>(arow + c), gv = *reinterpret_cast<const float4 *>(row + c);
          *reinterpret_cast<float4 *>(row + c) = make_float4(fix(gv.x, av.x), fix(gv.y, av.y), fix(gv.z, av.z), fix(gv.w, av.w));
        }
      } else {
        for (int c = lane; c < P; c += 64) row[c] = fix(row[c], arow[c]);
      }
    } else {
      const HardRef h = hard_ref(a, s, (int)t, T, P);
      if (!h.scores) continue;
      if (!a.cls) {
        if (lane == 0) row[h.cls] -= l2_scale * a.b;
      } else {
        for (int c = lane; c < P; c += 64)
          if (a.cls[c] == h.cls) row[c] -= l2_scale * a.b;
      }
    }
  }
}

int boost_blocks(int64_t rows) {
  const int64_t b = (rows + kBoostThreads / 64 - 1) / (kBoostThreads / 64);
  return (int)(b < 1 ? 1 : b > kBoostBlocksMax ? kBoostBlocksMax : b);
}

bool boost_acc_ok(const BoostAcc &a, int P) {
  if ((a.ref != nullptr) == (a.acc != nullptr)) return false;  // exactly one form
  if (a.acc && (a.acc_stride < P || !aligned(a.acc, 4))) return false;
  if (!aligned(a.ref, 4) || !aligned(a.cls, 4) || !aligned(a.seq_frames, 4)) return false;
  if (a.cls && !a.ref) return false;
  return a.b == a.b && !__builtin_isinf(a.b);
}

}  // namespace

int launch_boost_rows(int dtype, const void *x_v, int64_t sb, int64_t st, float *out, int64_t out_stride, int S, int T, int cols,
                      const BoostAcc &a, hipStream_t stream) {
  if (!x_v || !out || out_stride < cols || !boost_acc_ok(a, cols)) return TC_ERR_INVALID_ARGUMENT;
  if (!channel_last_strides_ok(S, T, cols, sb, st)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntBoost);
  const bool dense = a.acc != nullptr;
  return with_elem(dtype, [&](auto e) -> int {
    using E = typename decltype(e)::type;
    using bits = typename Elem<E>::bits;
    constexpr int kN = BoostLane<E>::kN;
    const bool vec = cols >= kN && (S == 1 || sb % kN == 0) && (T == 1 || st % kN == 0) && out_stride % 4 == 0 && aligned(x_v, 16) &&
                     aligned(out, 16) && (!dense || (a.acc_stride % 4 == 0 && aligned(a.acc, 16)));
    const dim3 blocks(boost_blocks((int64_t)S * T)), threads(kBoostThreads);
    with_bools(
        [&](auto v, auto d) {
          hipLaunchKernelGGL((boost_rows_kernel<E, decltype(v)::value, decltype(d)::value>), blocks, threads, 0, stream,
                             static_cast<const bits *>(x_v), sb, st, out, out_stride, S, T, cols, a);
        },
        vec, dense);
    TC_HIP_CHECK(hipGetLastError());
    return TC_OK;
  });
}

int launch_boost_bct(int dtype, const void *in_bct, float *out, int64_t out_stride, int B, int Cn, int T, const BoostAcc &a,
                     hipStream_t stream) {
  if (!in_bct || !out || B <= 0 || Cn <= 0 || T <= 0 || out_stride < Cn || !boost_acc_ok(a, Cn)) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_grid_ok(B, T)) return TC_ERR_UNSUPPORTED;
  count_launch(kCntBoost);
  const bool dense = a.acc != nullptr;
  const int tc = std::min(kBoostTileTMax, T);
  const size_t lds = (size_t)kBoostTileC * (tc | 1) * sizeof(float);
  const dim3 blocks((Cn + kBoostTileC - 1) / kBoostTileC, B, (T + kBoostTileTMax - 1) / kBoostTileTMax), threads(kBoostTileThreads);
  return with_elem(dtype, [&](auto e) -> int {
    using E = typename decltype(e)::type;
    using bits = typename Elem<E>::bits;
    with_bools(
        [&](auto d) {
          hipLaunchKernelGGL((boost_bct_kernel<E, decltype(d)::value>), blocks, threads, lds, stream, static_cast<const bits *>(in_bct),
                             out, out_stride, B, Cn, T, a);
        },
        dense);
    TC_HIP_CHECK(hipGetLastError());
    return TC_OK;
  });
}

int launch_boost_l2_sum(const float *yb, int64_t yb_stride, int S, int T, int P, const BoostAcc &a, double *seq_y2,
                        hipStream_t stream) {
  if (!yb || !seq_y2 || S <= 0 || T <= 0 || yb_stride < P || !boost_acc_ok(a, P)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntBoost);
  const bool vec = a.acc && P % 4 == 0 && yb_stride % 4 == 0 && a.acc_stride % 4 == 0 && aligned(yb, 16) && aligned(a.acc, 16);
  with_bools(
      [&](auto d, auto v) {
        if constexpr (decltype(d)::value || !decltype(v)::value)
          hipLaunchKernelGGL((boost_l2_sum_kernel<decltype(d)::value, decltype(v)::value>), dim3(S), dim3(kFixThreads), 0, stream, yb,
                             yb_stride, S, T, P, a, seq_y2);
      },
      a.acc != nullptr, vec);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_boost_l2_grad(float *g, int64_t g_stride, int S, int T, int P, const BoostAcc &a, float l2_scale, hipStream_t stream) {
  if (!g || S <= 0 || T <= 0 || g_stride < P || !boost_acc_ok(a, P)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntBoost);
  const bool vec = a.acc && P % 4 == 0 && g_stride % 4 == 0 && a.acc_stride % 4 == 0 && aligned(g, 16) && aligned(a.acc, 16);
  with_bools(
      [&](auto d, auto v) {
        if constexpr (decltype(d)::value || !decltype(v)::value)
          hipLaunchKernelGGL((boost_l2_grad_kernel<decltype(d)::value, decltype(v)::value>), dim3(boost_blocks((int64_t)S * T)),
                             dim3(kBoostThreads), 0, stream, g, g_stride, S, T, P, a, l2_scale);
      },
      a.acc != nullptr, vec);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
