// Sampled paths scored on the device, for gfx950: the token sequence of every frame-level pdf path and its unit-cost
// Levenshtein distance to a reference (tc_paths_edit_distance), and the gradient of functions.sampled_risk_surrogate in one
// pass (tc_sampled_risk_grad).  include/torchain_hip.h states both rules; all of the first is integer arithmetic and the
// second fixes the order of every sum, so each has one answer.
//
// path_edit_kernel.  One wavefront owns one path, kPathEditWaves independent wavefronts share a workgroup: no barrier, no
// atomic, nothing passes between waves.
//   tokenise : the lanes stride the frames 64 at a time.  c_t = token_of_pdf[pdf_t]; collapse mode compares c_t with c_{t-1}
//              (the lane below, lane 0 with the last lane of the chunk before); start mode reads start_of_pdf[pdf_t].  The
//              emit flags go through a ballot, a lane's slot is the tokens emitted so far plus the set bits below it.  The
//              hypothesis h lies in global memory (the caller's `tokens` or the workspace): it has no bound.
//   distance : row by row over h, the reference along the lanes in chunks of 64; the previous row D[i-1][1..M] and the
//              reference lie in the wave's own LDS, slot j always touched by lane j % 64, so the wave needs no fence for
//              them.  With x_j = min(D[i-1][j] + 1, D[i-1][j-1] + (h_i != r_j)) and x_0 = i,
//                  D[i][j] = j + min_{k <= j} (x_k - k):
//              a prefix minimum over the wave in six shuffle steps, its last lane carried into the next chunk, as is
//              D[i-1][64 c] for the diagonal of the next chunk's first lane.  64 tokens of h are fetched at a time and
//              handed round by shuffle.
// sampled_risk_grad_kernel.  One thread owns one (sequence, frame): it walks the K samples, the first to name a pdf sums
// grad_output[s] * weight[s][k] in double over the samples that name it, in k order, and stores the sum rounded once.
#include <hip/hip_runtime.h>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kPathEditThreads = kPathEditWaves * 64;
constexpr int kBig = 1 << 29;  // above every distance; kBig + 1 and kBig - j stay in range

constexpr int kRiskGradThreads = 256;

__device__ __forceinline__ int clamp_frames(const int32_t *seq_frames, int s, int T) {
  if (!seq_frames) return T;
  const int f = seq_frames[s];
  return f < 0 ? 0 : (f > T ? T : f);
}

// inclusive prefix minimum over the 64 lanes
__device__ __forceinline__ int wave_prefix_min(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(v, off, 64);
    if (lane >= off) v = min(v, o);
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(kPathEditThreads) void path_edit_kernel(const PathEditParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t path = (int64_t)blockIdx.x * kPathEditWaves + wave;
  if (path >= p.paths) return;  // (wave-uniform, and the kernel has no barrier)
  const int s = (int)(path / p.K);
  const int T = clamp_frames(p.seq_frames, s, p.T), P = p.P;
  const int32_t *pdf = p.pdf + path * p.T;
  int32_t *tok = p.tokens + path * p.T;

  // ---- tokenise ----
  int n = 0, carry = -1;  // carry: c_{t-1} of the chunk's first lane (-1 in front of frame 0: equal to no token)
  bool bad = false;
  for (int c0 = 0; c0 < T; c0 += 64) {
    const int t = c0 + lane;
    const bool in = t < T;
    const int q = in ? pdf[t] : 0;
    const bool oob = in && (unsigned)q >= (unsigned)P;
    const int c = in && !oob ? p.token_of_pdf[q] : -1;
    bool emit;
    if (p.start_of_pdf) {
      emit = c >= 0 && p.start_of_pdf[q] != 0;
    } else {
      int before = __shfl_up(c, 1, 64);
      if (lane == 0) before = carry;
      carry = __shfl(c, 63, 64);
      emit = c >= 0 && c != before;
    }
    bad |= __ballot(oob) != 0;
    const unsigned long long mask = __ballot(emit);
    if (emit) tok[n + __popcll(mask & ((1ull << lane) - 1ull))] = c;  // (slot <= t)
    n += __popcll(mask);
  }
  if (bad) {
    if (lane == 0) {
      p.dist[path] = -1;
      p.len[path] = -1;
    }
    if (p.fill)
      for (int t = lane; t < p.T; t += 64) tok[t] = -1;
    return;
  }
  if (p.fill)
    for (int t = n + lane; t < p.T; t += 64) tok[t] = -1;
  if (lane == 0) p.len[path] = n;

  // ---- distance ----
  int M = 0;
  if (p.max_ref > 0) {
    M = p.ref_len[s];
    M = M < 0 ? 0 : (M > p.max_ref ? p.max_ref : M);
  }
  if (M == 0) {
    if (lane == 0) p.dist[path] = n;
    return;
  }
  const int R = (p.max_ref + 63) & ~63;
  int32_t *row = reinterpret_cast<int32_t *>(lds_raw) + (int64_t)wave * 2 * R;  // slot j: D[i-1][j + 1]
  int32_t *rf = row + R;
  const int32_t *ref = p.ref + (int64_t)s * p.max_ref;
  for (int j = lane; j < M; j += 64) {
    row[j] = j + 1;
    rf[j] = ref[j];
  }
  __threadfence_block();  // h was stored by other lanes of this wave
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int hs = i0 + lane < n ? tok[i0 + lane] : -1;
    const int cnt = min(64, n - i0);
    for (int ii = 0; ii < cnt; ++ii) {
      const int h = __shfl(hs, ii, 64), i = i0 + ii + 1;
      int diag = i - 1;  // D[i-1][j0]
      int best = i;      // min over k <= j0 of x_k - k
      for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;  // the lane's column is j + 1
        const bool in = j < M;
        const int up = in ? row[j] : kBig;
        int left = __shfl_up(up, 1, 64);
        if (lane == 0) left = diag;
        diag = __shfl(up, 63, 64);
        const int x = in ? min(up + 1, left + (h != rf[j] ? 1 : 0)) : kBig;
        const int v = min(wave_prefix_min(x - (j + 1), lane), best);
        best = __shfl(v, 63, 64);
        if (in) row[j] = v + j + 1;
      }
    }
  }
  if (lane == ((M - 1) & 63)) p.dist[path] = row[M - 1];
}

namespace {

// a double rounded to float32 towards the odd neighbour where it is not exact: rounding the result to nearest even at 16
// bits then gives the double's own nearest 16-bit value (float32 keeps more than two bits beyond either 16-bit format)
__device__ __forceinline__ float round_to_odd(double d) {
  float f = (float)d;
  if (!((double)f == d) && d == d) {
    uint32_t u = __float_as_uint(f);
    if (fabs((double)f) > fabs(d)) u -= 1;  // (towards zero: also infinity -> FLT_MAX)
    f = __uint_as_float(u | 1u);
  }
  return f;
}

template <typename E>
__device__ __forceinline__ typename Elem<E>::bits round_once(double d) {
  if constexpr (std::is_same<E, float>::value)
    return (float)d;
  else
    return Elem<E>::round(round_to_odd(d));
}

}  // namespace

template <typename E>
__global__ __launch_bounds__(kRiskGradThreads) void sampled_risk_grad_kernel(const SampledRiskGradParams p) {
  using bits = typename Elem<E>::bits;
  const int64_t idx = (int64_t)blockIdx.x * kRiskGradThreads + threadIdx.x;
  if (idx >= (int64_t)p.S * p.T) return;
  const int s = (int)(idx / p.T), t = (int)(idx % p.T);
  if (t >= clamp_frames(p.seq_frames, s, p.T)) return;
  const int K = p.K;
  const int32_t *q = p.pdf + (int64_t)s * K * p.T + t;  // sample k: q[k * T]
  const double *w = p.weight + (int64_t)s * K;
  const double go = p.grad_out[s];
  const bits *in = reinterpret_cast<const bits *>(p.input) + s * p.in_s + t * p.in_t;
  bits *out = reinterpret_cast<bits *>(p.grad) + s * p.g_s + t * p.g_t;
  for (int k = 0; k < K; ++k) {
    const int pdf = q[(int64_t)k * p.T];
    if ((unsigned)pdf >= (unsigned)p.C) continue;
    bool first = true;
    for (int j = 0; j < k && first; ++j) first = q[(int64_t)j * p.T] != pdf;
    if (!first) continue;
    const float y = Elem<E>::widen(in[pdf * p.in_c]);
    if (!(y >= -kOutputLimit && y <= kOutputLimit)) continue;  // (a NaN too: the element stays +0)
    double acc = 0.0;
    for (int j = k; j < K; ++j)
      if (q[(int64_t)j * p.T] == pdf) {
        double term = go * w[j];
        asm volatile("" : "+v"(term));  // (a product and a sum, not one fused operation)
        acc += term;
      }
    out[pdf * p.g_c] = round_once<E>(acc);
  }
}

int launch_path_edit(const PathEditParams &p, hipStream_t stream) {
  if (!p.pdf || !p.token_of_pdf || !p.dist || !p.len || !p.tokens || p.paths <= 0 || p.K <= 0 || p.T <= 0 || p.P <= 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (p.max_ref < 0 || (p.max_ref > 0 && (!p.ref || !p.ref_len))) return TC_ERR_INVALID_ARGUMENT;
  if (p.max_ref > kPathEditMaxRef) return TC_ERR_UNSUPPORTED;
  const int64_t blocks = (p.paths + kPathEditWaves - 1) / kPathEditWaves;
  if (blocks > 0x7fffffff) return TC_ERR_UNSUPPORTED;
  const size_t lds = path_edit_lds_bytes(p.max_ref);
  TC_HIP_CHECK(allow_dynamic_lds((const void *)path_edit_kernel, lds));
  count_launch(kCntPathEdit);
  hipLaunchKernelGGL(path_edit_kernel, dim3((unsigned)blocks), dim3(kPathEditThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_sampled_risk_grad(const SampledRiskGradParams &p, int dtype, hipStream_t stream) {
  if (!p.pdf || !p.weight || !p.grad_out || !p.input || !p.grad || p.S <= 0 || p.K <= 0 || p.T <= 0 || p.C <= 0)
    return TC_ERR_INVALID_ARGUMENT;
  const int64_t blocks = ((int64_t)p.S * p.T + kRiskGradThreads - 1) / kRiskGradThreads;
  if (blocks > 0x7fffffff) return TC_ERR_UNSUPPORTED;
  return with_elem(dtype, [&](auto tag) -> int {
    using E = typename decltype(tag)::type;
    count_launch(kCntSampledRiskGrad);
    hipLaunchKernelGGL(sampled_risk_grad_kernel<E>, dim3((unsigned)blocks), dim3(kRiskGradThreads), 0, stream, p);
    TC_HIP_CHECK(hipGetLastError());
    return TC_OK;
  });
}

}  // namespace tc
