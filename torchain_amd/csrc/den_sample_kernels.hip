// Paths drawn from the denominator graph's own path posterior, for gfx950 (tc_den_sample_paths): exact samples of
// P(path | y) under the model of tc_den_forward_backward -- p_t(j) = exp(clamp(y_t(j), +-kOutputLimit)), the graph's
// initial probabilities pi, every state final, and the leaky-HMM transitions.  It is den_best_path_kernels.hip with a draw
// where that one maximises: a forward pass that keeps alpha, then a traceback that finds every choice again from the
// stored alpha.  No back-pointers, no random numbers made here: the caller gives the uniforms.
//
// The model (the forward half of den_accuracy_kernels.hip without A), c the leaky-HMM coefficient:
//     alpha_0 = pi;   asum_t = sum_h alpha_t(h);   alpha'_t(h) = alpha_t(h) + c pi(h) asum_t
//     alpha_{t+1}(g) = sum_{h->g} alpha'_t(h) w p_t(pdf) / asum_t
// A latent path has levels t = 0 .. T; at each it holds the state it entered, pre_t, and the state it leaves from, post_t,
// which differ where a leak happened.  With u = uniforms[s, k] (float32 in [0, 1), (T_max + 1, 3)):
//     pick(weights, u): the first index, in list order, whose inclusive cumulative sum exceeds u * total; when rounding
//                       leaves none, the last index of positive weight.  A zero weight is never picked.  Doubles throughout.
//     post_T = pick(alpha'_T over the states, u[T, 2])
//     for t = T .. 0, j = post_t:
//         no leak iff u[t, 0] * alpha'_t(j) < alpha_t(j);   pre_t = j, or with a leak pick(alpha_t over the states, u[t, 1])
//         t > 0: the in-arcs of pre_t in the tables' order (the graph's arc list within a destination), each weighted
//                alpha'_{t-1}(src) * w * p_{t-1}(pdf) (the frame's 1 / asum is common to the list), picked with u[t-1, 2]:
//                pdf_{t-1} is that arc's pdf, post_{t-1} its source.
// A sequence with a NaN or +-inf in its valid frames (the accuracy kernel's scan), or with an asum_t that is zero,
// subnormal or not finite, or with sum alpha'_T = 0, gets -1 in every slot; the others keep their bits.  Padding slots
// are -1.
//
// Arithmetic.  alpha_t and asum_t are float32 where they are stored; every sum over arcs or states is accumulated in
// double and rounded once when it is stored.  p_t(j) is the float32 expf.  alpha'_t(h) is never stored: it is
// (float)((double)alpha_t(h) + (double)pi(h) * (c * (double)asum_t)) wherever it is needed (leak_alpha), in the forward
// pass and in the traceback alike, so the traceback's weights are the forward pass's terms bit for bit.  The forward
// term of an arc is the double product alpha'(src) * (w * p); the new alpha is the double sum times 1 / asum_t.
//
// One workgroup of 16 wavefronts owns one sequence, one launch does everything:
//   scan     : every y of the sequence's valid frames is looked at.
//   forward  : frame by frame, lane = destination state walks its in-arcs (a row of more than kLongRow arcs by its whole
//              wave); alpha_t of every frame and asum_t go to the workspace.  RESIDENT: alpha'_t of the frame being read
//              is in LDS; otherwise it is formed from the workspace's row per arc, by the same expression: the same bits.
//   traceback: the 16 waves take the K samples, wave w the samples w, w + 16, ...  A pick is wave-wide: the list in
//              chunks of 64, lane = item, an inclusive double prefix over the wave on top of the chunks before, and the
//              first crossing lane by ballot.  (Any association of the double sums serves: it moves a threshold by about
//              1e-16 of the total.)
// The tables are the graph's (den_acc_tables; the training tables are not read), the orders are fixed, nothing is atomic:
// a sequence's output depends on its own rows of y and of the uniforms, the graph and c alone, and a sample on its own
// uniforms alone.
#include <float.h>
#include <math.h>

#include "chain_internal.h"

namespace tc {

namespace {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / 64;
constexpr int kLongRow = 128;  // arcs beyond which a state's list is walked by its whole wave

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// inclusive prefix sums over the 64 lanes
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// the sum of a over the workgroup, in every thread: wave butterflies, then the wave sums in wave order.  Both barriers are
// the caller's too: what was stored before the call is visible after it.
__device__ __forceinline__ double block_sum(double a, double *red, int lane, int wave) {
  a = wave_sum(a);
  __syncthreads();  // (the slots' readers of the call before)
  if (lane == 0) red[wave] = a;
  __syncthreads();
  a = 0.0;
#pragma unroll
  for (int w = 0; w < kSampleWaves; ++w) a += red[w];
  return a;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

// whether any y of the sequence's T valid frames is a NaN or an infinity (every thread gets the answer): the accuracy
// kernel's scan.  slot: kSampleWaves ints of LDS that the next user puts a barrier in front of.  (Not __syncthreads_or:
// it brings static LDS with it, which moves the base of the dynamic region.)
__device__ __forceinline__ bool scan_bad(const float *y, int64_t y_stride, int S, int P, int q, int T, int lane, int wave, int *slot) {
  int bad = 0;
  for (int t = wave; t < T; t += kSampleWaves) {
    const float *row = y + ((int64_t)t * S + q) * y_stride;
    for (int c = lane; c < P; c += 64) bad |= !finite(row[c]);
  }
  const int any = __ballot(bad != 0) != 0;
  if (lane == 0) slot[wave] = any;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < kSampleWaves; ++w) all |= slot[w];
  return all != 0;
}

// alpha'_t(h) from what is stored, ca = c * asum_t: the one expression, forward and traceback alike
__device__ __forceinline__ float leak_alpha(float alpha, float pi, double ca) { return (float)((double)alpha + (double)pi * ca); }

__device__ __forceinline__ float clamped_exp(float y) { return expf(fminf(fmaxf(y, -kOutputLimit), kOutputLimit)); }

__device__ __forceinline__ bool asum_ok(float asum) { return asum >= FLT_MIN && asum <= FLT_MAX; }

// pick(weights, u) by one wave, weight(i) the non-negative double weight of item i of n (n, u and the weights are the same
// in every lane); every lane returns the index, -1 when the total is not positive
template <typename W>
__device__ __forceinline__ int wave_pick(int n, float u, int lane, W weight) {
  double base = 0.0, w = 0.0, cum = 0.0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    w = c0 + lane < n ? weight(c0 + lane) : 0.0;
    cum = base + wave_scan(w, lane);
    base = __shfl(cum, 63, 64);
  }
  if (!(base > 0.0)) return -1;
  const double thr = (double)u * base;
  if (n <= 64) {  // (the one chunk is still in the registers)
    const unsigned long long over = __ballot(w > 0.0 && cum > thr);
    if (over) return __ffsll((long long)over) - 1;
    return 63 - __clzll((long long)__ballot(w > 0.0));
  }
  int last = -1;
  base = 0.0;
  for (int c0 = 0; c0 < n; c0 += 64) {  // the same sums again, bit for bit
    w = c0 + lane < n ? weight(c0 + lane) : 0.0;
    cum = base + wave_scan(w, lane);
    base = __shfl(cum, 63, 64);
    const unsigned long long over = __ballot(w > 0.0 && cum > thr);
    if (over) return c0 + __ffsll((long long)over) - 1;
    const unsigned long long pos = __ballot(w > 0.0);
    if (pos) last = c0 + 63 - __clzll((long long)pos);
  }
  return last;
}

}  // namespace

// RAGGED: the loop bound is the sequence's own.  RESIDENT: see above.
template <bool RAGGED, bool RESIDENT>
__global__ __launch_bounds__(kSampleThreads) void den_sample_kernel(const DenSampleParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *red = reinterpret_cast<double *>(lds_raw);                         // [kSampleWaves]
  float *lds_ap = reinterpret_cast<float *>(lds_raw + kDenSampleSmallLds);   // RESIDENT: alpha'_t, [Hs]

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int H = p.H, S = p.S, Hs = p.Hs, K = p.K;
  const float *pi = p.t.pi;
  const int32_t *in_begin = p.t.in_begin;
  const DenAccArc *in_arcs = p.t.in_arcs;
  const double c = (double)p.leaky;
  int32_t *pdf_seq = p.pdf_out + (int64_t)q * K * p.T;
  int32_t *state_seq = p.state_out ? p.state_out + (int64_t)q * K * (p.T + 1) * 2 : nullptr;
  float *hist = reinterpret_cast<float *>(p.workspace) + (int64_t)q * den_sample_seq_floats(H, p.T);
  float *asums = hist + (int64_t)(p.T + 1) * Hs;

  // -1 in the slots t >= from (pdfs) and t >= from + 1 (states) of every sample, by the whole workgroup
  auto blank = [&](int from) {
    const int n = p.T - from;
    for (int64_t i = tid; i < (int64_t)K * n; i += kSampleThreads) pdf_seq[(i / n) * p.T + from + i % n] = -1;
    if (state_seq)
      for (int64_t i = tid; i < (int64_t)K * n * 2; i += kSampleThreads)
        state_seq[(i / (2 * n)) * (p.T + 1) * 2 + (int64_t)(from + 1) * 2 + i % (2 * n)] = -1;
  };
  if (T < p.T) blank(T);  // a ragged batch's padding slots
  auto no_paths = [&]() {
    for (int64_t i = tid; i < (int64_t)K * T; i += kSampleThreads) pdf_seq[(i / T) * p.T + i % T] = -1;
    if (state_seq)
      for (int64_t i = tid; i < (int64_t)K * (T + 1) * 2; i += kSampleThreads)
        state_seq[(i / (2 * (T + 1))) * (p.T + 1) * 2 + i % (2 * (T + 1))] = -1;
  };

  // ---- scan ----
  if (scan_bad(p.y, p.y_stride, S, p.P, q, T, lane, wave, reinterpret_cast<int *>(red))) return no_paths();

  // ---- forward: row t of the history is alpha_t ----
  double sa = 0.0;
  for (int h = tid; h < H; h += kSampleThreads) {
    hist[h] = pi[h];
    sa += (double)pi[h];
  }
  sa = block_sum(sa, red, lane, wave);
  for (int t = 0;; ++t) {
    const float asum = (float)sa;  // (the same in every thread)
    if (tid == 0) asums[t] = asum;
    if (!asum_ok(asum)) return no_paths();
    if (t == T) break;
    const double ca = c * (double)asum, inv = 1.0 / (double)asum;
    const float *row = hist + (int64_t)t * Hs;
    float *next = hist + (int64_t)(t + 1) * Hs;
    const float *yrow = p.y + ((int64_t)t * S + q) * p.y_stride;
    if (RESIDENT) {
      for (int h = tid; h < H; h += kSampleThreads) lds_ap[h] = leak_alpha(row[h], pi[h], ca);
      __syncthreads();
    }
    sa = 0.0;
    for (int base = wave * 64; base < H; base += kSampleThreads) {  // (wave-uniform: the shuffles below see all lanes)
      const int h = base + lane;
      int b = 0, e = 0;
      if (h < H) {
        b = in_begin[h];
        e = in_begin[h + 1];
      }
      auto term = [&](int i) {
        const DenAccArc a = in_arcs[i];
        const float ap = RESIDENT ? lds_ap[a.other] : leak_alpha(row[a.other], pi[a.other], ca);
        return (double)ap * ((double)a.w * (double)clamped_exp(yrow[a.pdf]));
      };
      const bool long_row = e - b > kLongRow;
      double acc = 0.0;
      if (!long_row)
        for (int i = b; i < e; ++i) acc += term(i);
      unsigned long long todo = __ballot(long_row);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
        double w = 0.0;
        for (int i = bb + lane; i < ee; i += 64) w += term(i);
        w = wave_sum(w);
        if (lane == l) acc = w;
      }
      if (h < H) {
        const float na = (float)(acc * inv);
        next[h] = na;
        sa += (double)na;
      }
    }
    sa = block_sum(sa, red, lane, wave);  // (its barriers: row t + 1 is visible, alpha'_t in LDS is read)
  }
  __syncthreads();  // (asum_T)

  // ---- traceback: one wave a sample ----
  for (int k = wave; k < K; k += kSampleWaves) {
    const float *u = p.uniforms + ((int64_t)q * K + k) * (p.T + 1) * 3;
    int32_t *pdf_o = pdf_seq + (int64_t)k * p.T;
    int32_t *state_o = state_seq ? state_seq + (int64_t)k * (p.T + 1) * 2 : nullptr;
    bool ok = true;
    int post;
    {
      const float *row = hist + (int64_t)T * Hs;
      const double ca = c * (double)asums[T];
      post = wave_pick(H, u[(int64_t)T * 3 + 2], lane, [&](int i) { return (double)leak_alpha(row[i], pi[i], ca); });
      ok = post >= 0;
    }
    for (int t = T; ok; --t) {
      const float *row = hist + (int64_t)t * Hs;
      const float al = row[post], ap = leak_alpha(al, pi[post], c * (double)asums[t]);
      int pre = post;
      if (!((double)u[(int64_t)t * 3] * (double)ap < (double)al)) {  // (wave-uniform)
        pre = wave_pick(H, u[(int64_t)t * 3 + 1], lane, [&](int i) { return (double)row[i]; });
        if (pre < 0) ok = false;  // (not reached: asum_t is positive)
      }
      if (!ok) break;
      if (state_o && lane == 0) {
        state_o[2 * t] = pre;
        state_o[2 * t + 1] = post;
      }
      if (t == 0) break;
      const float *prev = row - Hs;
      const double ca = c * (double)asums[t - 1];
      const float *yrow = p.y + ((int64_t)(t - 1) * S + q) * p.y_stride;
      const int b = in_begin[pre], n = in_begin[pre + 1] - b;
      const int i = wave_pick(n, u[(int64_t)(t - 1) * 3 + 2], lane, [&](int j) {
        const DenAccArc a = in_arcs[b + j];
        return (double)leak_alpha(prev[a.other], pi[a.other], ca) * ((double)a.w * (double)clamped_exp(yrow[a.pdf]));
      });
      if (i < 0) {  // (not reached: alpha_t(pre_t) > 0 is the sum of these)
        ok = false;
        break;
      }
      const DenAccArc a = in_arcs[b + i];
      if (lane == 0) pdf_o[t - 1] = a.pdf;
      post = a.other;
    }
    if (!ok) {
      for (int t = lane; t < T; t += 64) pdf_o[t] = -1;
      if (state_o)
        for (int t = lane; t < 2 * (T + 1); t += 64) state_o[t] = -1;
    }
  }
}

namespace {

template <bool RAGGED, bool RESIDENT>
int launch_sample(const DenSampleParams &p, hipStream_t stream) {
  void (*kernel)(const DenSampleParams) = den_sample_kernel<RAGGED, RESIDENT>;
  const size_t lds = kDenSampleSmallLds + (RESIDENT ? (size_t)4 * p.Hs : 0);
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kSampleThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

int launch_den_sample_paths(const DenSampleParams &p, hipStream_t stream) {
  if (!p.y || !p.uniforms || !p.pdf_out || !p.workspace || !p.t.in_arcs || p.K <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (p.resident && !den_sample_resident(p.H)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenSample);
  if (!p.resident) count_launch(kCntDenSampleStreamed);
  if (p.seq_frames) return p.resident ? launch_sample<true, true>(p, stream) : launch_sample<true, false>(p, stream);
  return p.resident ? launch_sample<false, true>(p, stream) : launch_sample<false, false>(p, stream);
}

}  // namespace tc
