// The cross-entropy head's log-softmax folded into the training step (tc_chain_step_log_softmax).
//
// Kaldi's chain recipes end the cross-entropy head in a log-softmax ("output-xent"), take the objective
// sum(xent_output * xent_deriv) on its log-probabilities and back-propagate xent_regularize * xent_deriv through it
// ([K] nnet-chain-training.cc).  The reference has no log-softmax in training (its head ends in a Conv1d; a TODO at
// torchain/functions.py:88-89; forward.py:67 applies log_softmax at inference only).  With the option the step does both
// ends of it in two passes of its own:
//   the row statistics (in front of the objective): (max, log(sum(exp(x - max)))) of every row of xent_input, which the
//     numerators subtract from x in their cross-entropy sums (NumParams::xent_lse);
//   the gradient pass (behind the objective and its soft-failure reset, in front of the last passes): the xent gradient V
//     the numerator left becomes G = V - rowsum(V) * softmax(x), in place, in float32.
// Two address forms each: rows with unit channel stride (float32 2-D tensors, and the widened / gathered float32 scratch of
// 16-bit 2-D tensors and channel-last views), a wave per row for the statistics and a workgroup per row for the gradient;
// and the caller's (B, C, T) tensor, channel stride T, lanes over frames and waves over channels, a tile of 64 frames per
// workgroup.  Every sum has one order: the results do not depend on the run.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {
namespace {

constexpr int kRowThreads = 256, kRowWaves = kRowThreads / 64;
// float4 of a row that a thread of the row kernels loads in one batch (and the gradient pass keeps in registers between its
// two passes): 4 * 256 float4 = a row of 4096 channels; what lies behind goes through the loops that follow
constexpr int kRowBatch = 4;
constexpr int kTileFrames = 64, kBctWaves = 8, kBctThreads = kTileFrames * kBctWaves;

// running (max, sum(exp(x - max))) of the elements seen so far; s == 0: none yet.  The exponentials are float32; they are
// added four at a time in float32 and from there on in double: a thread of the (B, C, T) form adds a thousand and more of
// them in a row, and in float32 that chain alone cost more than the whole of the rest (measured against float64: the
// log-sum's error scales every element of the row's softmax).
struct MaxSum {
  float m;
  double s;
};

// A non-finite element makes the row's s NaN, and with it every element of the row's gradient and its objective term: the
// 0 * x terms are 0 for a finite x and NaN for NaN and +-inf (fmaxf alone passes a NaN by, and exp(-inf) is a plain 0).
__device__ __forceinline__ float poison(float x) { return 0.0f * x; }
__device__ __forceinline__ void ms_add4(MaxSum &a, float x0, float x1, float x2, float x3) {
  const float m = fmaxf(fmaxf(fmaxf(x0, x1), fmaxf(x2, x3)), a.m);
  a.s = a.s * (double)expf(a.m - m) + (double)(((expf(x0 - m) + expf(x1 - m)) + (expf(x2 - m) + expf(x3 - m))) +
                                               ((poison(x0) + poison(x1)) + (poison(x2) + poison(x3))));
  a.m = m;
}
__device__ __forceinline__ void ms_add(MaxSum &a, float x) {
  const float m = fmaxf(x, a.m);
  a.s = a.s * (double)expf(a.m - m) + (double)(expf(x - m) + poison(x));
  a.m = m;
}
__device__ __forceinline__ MaxSum ms_merge(MaxSum a, MaxSum b) {
  if (b.s == 0.0) return a;
  if (a.s == 0.0) return b;
  const float m = fmaxf(a.m, b.m);
  MaxSum r;
  r.m = m;
  r.s = a.s * (double)expf(a.m - m) + b.s * (double)expf(b.m - m);
  return r;
}
// (an empty share starts at the lowest finite value, so that its first element forms exp(0), not exp(-inf + inf))
__device__ __forceinline__ MaxSum ms_empty() { return MaxSum{-3.402823466e38f, 0.0}; }
// the row's second statistic: log(sum(exp(x - max))), rounded once
__device__ __forceinline__ float ms_log(const MaxSum &a) { return (float)log(a.s); }

__device__ __forceinline__ bool row_live(const int32_t *live_frames, int s, int t) {
  return !live_frames || t < live_frames[s];
}

// ---- rows with unit channel stride: one workgroup per row --------------------------------------------------------------

// (a wave per row, four rows a workgroup: no barrier and no LDS between a row's loads and its two statistics)
template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void row_stats_kernel(const float *__restrict__ x, int64_t x_stride, int64_t rows,
                                                                int P, float *__restrict__ stats) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * kRowWaves) {
    const float *xr = x + row * x_stride;
    MaxSum a = ms_empty();
    int c0 = 0;
    if constexpr (VEC) {
      const int n4 = P >> 2;
      const float4 *x4 = reinterpret_cast<const float4 *>(xr);
      // (a batch of loads at clamped indices in front of the arithmetic: a load under a condition would be waited for alone)
      for (int i0 = lane; i0 < n4; i0 += kRowBatch * 64) {
        float4 v[kRowBatch];
#pragma unroll
        for (int k = 0; k < kRowBatch; ++k) v[k] = x4[min(i0 + k * 64, n4 - 1)];
#pragma unroll
        for (int k = 0; k < kRowBatch; ++k)
          if (i0 + k * 64 < n4) ms_add4(a, v[k].x, v[k].y, v[k].z, v[k].w);
      }
      c0 = n4 << 2;
    }
    for (int c = c0 + lane; c < P; c += 64) ms_add(a, xr[c]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      MaxSum b;
      b.m = __shfl_xor(a.m, off, 64);
      b.s = __shfl_xor(a.s, off, 64);
      // (both lanes of a pair form the same sum: the lower lane's share first)
      a = (lane & off) ? ms_merge(b, a) : ms_merge(a, b);
    }
    if (lane == 0) {
      stats[2 * row] = a.m;
      stats[2 * row + 1] = ms_log(a);
    }
  }
}

// G = V - rowsum(V) * exp((x - max) - log sum), or +0 for a row of V without a non-zero entry
__device__ __forceinline__ float grad_elem(bool mass, float v, float msum, float x, float mx, float ls) {
  return mass ? v - msum * expf((x - mx) - ls) : 0.0f;
}

template <bool VEC>
__global__ __launch_bounds__(kRowThreads) void row_grad_kernel(const float *__restrict__ x, int64_t x_stride, float *g,
                                                               int64_t g_stride, int S, int64_t rows, int P,
                                                               const float *__restrict__ stats,
                                                               const int32_t *__restrict__ live_frames) {
  __shared__ float sh_sum[kRowWaves];
  __shared__ int sh_nz[kRowWaves];
  const int tid = threadIdx.x;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    if (!row_live(live_frames, (int)(row % S), (int)(row / S))) continue;  // (the whole workgroup: one row)
    const float *xr = x + row * x_stride;
    float *gr = g + row * g_stride;
    const int n4 = VEC ? P >> 2 : 0;
    float sum = 0.0f;
    int nz = 0;
    float4 vc[kRowBatch], xc[kRowBatch];  // the thread's first float4 of V and of x, held across the barrier
    if constexpr (VEC) {
      const float4 *g4 = reinterpret_cast<const float4 *>(gr), *x4 = reinterpret_cast<const float4 *>(xr);
#pragma unroll
      for (int k = 0; k < kRowBatch; ++k) vc[k] = g4[min(tid + k * kRowThreads, n4 - 1)];
#pragma unroll
      for (int k = 0; k < kRowBatch; ++k) xc[k] = x4[min(tid + k * kRowThreads, n4 - 1)];
#pragma unroll
      for (int k = 0; k < kRowBatch; ++k)
        if (tid + k * kRowThreads < n4) {
          sum += (vc[k].x + vc[k].y) + (vc[k].z + vc[k].w);
          nz |= (vc[k].x != 0.0f) | (vc[k].y != 0.0f) | (vc[k].z != 0.0f) | (vc[k].w != 0.0f);
        }
      for (int i = tid + kRowBatch * kRowThreads; i < n4; i += kRowThreads) {
        const float4 v = g4[i];
        sum += (v.x + v.y) + (v.z + v.w);
        nz |= (v.x != 0.0f) | (v.y != 0.0f) | (v.z != 0.0f) | (v.w != 0.0f);
      }
    }
    for (int c = (n4 << 2) + tid; c < P; c += kRowThreads) {
      const float v = gr[c];
      sum += v;
      nz |= v != 0.0f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum += __shfl_xor(sum, off, 64);
      nz |= __shfl_xor(nz, off, 64);
    }
    if ((tid & 63) == 0) {
      sh_sum[tid >> 6] = sum;
      sh_nz[tid >> 6] = nz;
    }
    __syncthreads();
    float msum = sh_sum[0];
    int any = sh_nz[0];
    for (int w = 1; w < kRowWaves; ++w) {
      msum += sh_sum[w];
      any |= sh_nz[w];
    }
    const bool mass = any != 0;
    const float mx = stats[2 * row], ls = stats[2 * row + 1];
    // (channels behind the first 4096, and rows without float4: the second read of V comes from the cache, the workgroup
    // has just read these bytes)
    if constexpr (VEC) {
      const float4 *x4 = reinterpret_cast<const float4 *>(xr);
      float4 *g4 = reinterpret_cast<float4 *>(gr);
#pragma unroll
      for (int k = 0; k < kRowBatch; ++k)
        if (tid + k * kRowThreads < n4) {
          float4 o;
          o.x = grad_elem(mass, vc[k].x, msum, xc[k].x, mx, ls);
          o.y = grad_elem(mass, vc[k].y, msum, xc[k].y, mx, ls);
          o.z = grad_elem(mass, vc[k].z, msum, xc[k].z, mx, ls);
          o.w = grad_elem(mass, vc[k].w, msum, xc[k].w, mx, ls);
          g4[tid + k * kRowThreads] = o;
        }
      for (int i = tid + kRowBatch * kRowThreads; i < n4; i += kRowThreads) {
        const float4 xv = x4[i], v = g4[i];
        float4 o;
        o.x = grad_elem(mass, v.x, msum, xv.x, mx, ls);
        o.y = grad_elem(mass, v.y, msum, xv.y, mx, ls);
        o.z = grad_elem(mass, v.z, msum, xv.z, mx, ls);
        o.w = grad_elem(mass, v.w, msum, xv.w, mx, ls);
        g4[i] = o;
      }
    }
    for (int c = (n4 << 2) + tid; c < P; c += kRowThreads) gr[c] = grad_elem(mass, gr[c], msum, xr[c], mx, ls);
    __syncthreads();
  }
}

// ---- the caller's (B, C, T) tensor: lanes over frames, waves over channels ---------------------------------------------

template <typename E>
__global__ __launch_bounds__(kBctThreads) void bct_stats_kernel(const float *__restrict__ x, int S, int T, int P,
                                                                float *__restrict__ stats) {
  __shared__ float sh_m[kBctWaves][kTileFrames];
  __shared__ double sh_s[kBctWaves][kTileFrames];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = blockIdx.x * kTileFrames + lane;
  const bool in = t < T;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    MaxSum a = ms_empty();
    if (in) {
      const int64_t base = (int64_t)s * P * T + t;
      int c = w;
      for (; c + 3 * kBctWaves < P; c += 4 * kBctWaves) {
        const float x0 = load_elem<E>(x, base + (int64_t)c * T), x1 = load_elem<E>(x, base + (int64_t)(c + kBctWaves) * T),
                    x2 = load_elem<E>(x, base + (int64_t)(c + 2 * kBctWaves) * T),
                    x3 = load_elem<E>(x, base + (int64_t)(c + 3 * kBctWaves) * T);
        ms_add4(a, x0, x1, x2, x3);
      }
      for (; c < P; c += kBctWaves) ms_add(a, load_elem<E>(x, base + (int64_t)c * T));
    }
    sh_m[w][lane] = a.m;
    sh_s[w][lane] = a.s;
    __syncthreads();
    if (w == 0 && in) {
      MaxSum r{sh_m[0][lane], sh_s[0][lane]};
      for (int k = 1; k < kBctWaves; ++k) r = ms_merge(r, MaxSum{sh_m[k][lane], sh_s[k][lane]});
      const int64_t row = (int64_t)t * S + s;
      stats[2 * row] = r.m;
      stats[2 * row + 1] = ms_log(r);
    }
    __syncthreads();
  }
}

template <typename E>
__global__ __launch_bounds__(kBctThreads) void bct_grad_kernel(const float *__restrict__ x, float *g, int S, int T, int P,
                                                               const float *__restrict__ stats,
                                                               const int32_t *__restrict__ live_frames) {
  __shared__ float sh_sum[kBctWaves][kTileFrames];
  __shared__ int sh_nz[kBctWaves][kTileFrames];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = blockIdx.x * kTileFrames + lane;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    const bool live = t < T && row_live(live_frames, s, t);
    const int64_t base = (int64_t)s * P * T + t;
    float sum = 0.0f;
    int nz = 0;
    if (live) {
      int c = w;
      for (; c + 3 * kBctWaves < P; c += 4 * kBctWaves) {
        const float v0 = g[base + (int64_t)c * T], v1 = g[base + (int64_t)(c + kBctWaves) * T],
                    v2 = g[base + (int64_t)(c + 2 * kBctWaves) * T], v3 = g[base + (int64_t)(c + 3 * kBctWaves) * T];
        sum += (v0 + v1) + (v2 + v3);
        nz |= (v0 != 0.0f) | (v1 != 0.0f) | (v2 != 0.0f) | (v3 != 0.0f);
      }
      for (; c < P; c += kBctWaves) {
        const float v = g[base + (int64_t)c * T];
        sum += v;
        nz |= v != 0.0f;
      }
    }
    sh_sum[w][lane] = sum;
    sh_nz[w][lane] = nz;
    __syncthreads();
    if (live) {
      float msum = sh_sum[0][lane];
      int any = sh_nz[0][lane];
      for (int k = 1; k < kBctWaves; ++k) {
        msum += sh_sum[k][lane];
        any |= sh_nz[k][lane];
      }
      const bool mass = any != 0;
      const int64_t row = (int64_t)t * S + s;
      const float mx = stats[2 * row], ls = stats[2 * row + 1];
      int c = w;
      for (; c + 3 * kBctWaves < P; c += 4 * kBctWaves) {
        const int64_t i0 = base + (int64_t)c * T, i1 = base + (int64_t)(c + kBctWaves) * T,
                      i2 = base + (int64_t)(c + 2 * kBctWaves) * T, i3 = base + (int64_t)(c + 3 * kBctWaves) * T;
        const float x0 = load_elem<E>(x, i0), x1 = load_elem<E>(x, i1), x2 = load_elem<E>(x, i2), x3 = load_elem<E>(x, i3);
        const float v0 = g[i0], v1 = g[i1], v2 = g[i2], v3 = g[i3];
        g[i0] = grad_elem(mass, v0, msum, x0, mx, ls);
        g[i1] = grad_elem(mass, v1, msum, x1, mx, ls);
        g[i2] = grad_elem(mass, v2, msum, x2, mx, ls);
        g[i3] = grad_elem(mass, v3, msum, x3, mx, ls);
      }
      for (; c < P; c += kBctWaves) {
        const int64_t i = base + (int64_t)c * T;
        g[i] = grad_elem(mass, g[i], msum, load_elem<E>(x, i), mx, ls);
      }
    }
    __syncthreads();
  }
}

bool rows_vec(const void *p, int64_t stride) { return stride % 4 == 0 && aligned(p, 16); }  // (asked with P >= 4 only)

}  // namespace

int launch_xent_row_stats(int dtype, const void *x, int x_bct, int64_t x_stride, int S, int T, int P, float *stats,
                          hipStream_t stream) {
  if (!x || !stats || S <= 0 || T <= 0 || P <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (!x_bct && (dtype != TC_DTYPE_F32 || x_stride < P)) return TC_ERR_INVALID_ARGUMENT;  // (rows are float32)
  count_launch(kCntXentLogSoftmax);
  const float *xf = static_cast<const float *>(x);
  if (x_bct) {
    const dim3 blocks((unsigned)((T + kTileFrames - 1) / kTileFrames), (unsigned)std::min(S, 65535)), threads(kBctThreads);
    const int rc = with_elem(dtype, [&](auto e) {
      hipLaunchKernelGGL(bct_stats_kernel<typename decltype(e)::type>, blocks, threads, 0, stream, xf, S, T, P, stats);
      return TC_OK;
    });
    if (rc != TC_OK) return rc;
  } else {
    const int64_t rows = (int64_t)S * T;
    const dim3 blocks((unsigned)std::min<int64_t>((rows + kRowWaves - 1) / kRowWaves, (int64_t)1 << 20)), threads(kRowThreads);
    if (P >= 4 && rows_vec(x, x_stride))
      hipLaunchKernelGGL(row_stats_kernel<true>, blocks, threads, 0, stream, xf, x_stride, rows, P, stats);
    else
      hipLaunchKernelGGL(row_stats_kernel<false>, blocks, threads, 0, stream, xf, x_stride, rows, P, stats);
  }
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_xent_softmax_grad(int dtype, const void *x, int x_bct, int64_t x_stride, float *g, int64_t g_stride, int S, int T,
                             int P, const float *stats, const int32_t *live_frames, hipStream_t stream) {
  if (!x || !g || !stats || S <= 0 || T <= 0 || P <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (!x_bct && (dtype != TC_DTYPE_F32 || x_stride < P || g_stride < P)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntXentLogSoftmax);
  const float *xf = static_cast<const float *>(x);
  if (x_bct) {
    const dim3 blocks((unsigned)((T + kTileFrames - 1) / kTileFrames), (unsigned)std::min(S, 65535)), threads(kBctThreads);
    const int rc = with_elem(dtype, [&](auto e) {
      hipLaunchKernelGGL(bct_grad_kernel<typename decltype(e)::type>, blocks, threads, 0, stream, xf, g, S, T, P, stats,
                         live_frames);
      return TC_OK;
    });
    if (rc != TC_OK) return rc;
  } else {
    const int64_t rows = (int64_t)S * T;
    const dim3 blocks((unsigned)std::min<int64_t>(rows, (int64_t)1 << 20)), threads(kRowThreads);
    if (P >= 4 && rows_vec(x, x_stride) && rows_vec(g, g_stride))
      hipLaunchKernelGGL(row_grad_kernel<true>, blocks, threads, 0, stream, xf, x_stride, g, g_stride, S, rows, P, stats,
                         live_frames);
    else
      hipLaunchKernelGGL(row_grad_kernel<false>, blocks, threads, 0, stream, xf, x_stride, g, g_stride, S, rows, P, stats,
                         live_frames);
  }
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
