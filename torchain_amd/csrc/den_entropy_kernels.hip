// Entropy of the denominator graph's path posterior and its gradient, for gfx950 (tc_den_path_entropy):
//
//     H_s = - sum_paths P(path | y_s) log P(path | y_s) = log Z_s - E_s[log W]
//
// over the LATENT paths of the denominator's own model (den_sample_kernels.hip draws from it): p_t(j) = exp(yh_t(j)),
// yh = clamp(y, +-kOutputLimit), the graph's initial probabilities pi, the leaky-HMM coefficient c, every state final.  A path
// holds (pre_t, post_t) at every level t = 0 .. T and an arc at every frame;
//     W(path) = pi(pre_0) prod_{t<=T} lambda_t prod_{t<T} w_a p_t(pdf_a),   lambda_t = 1 (no leak) or c pi(post_t) (a leak).
// E[log W] is a first-order and dH/dy a second-order expectation: the forward-backward below runs in the expectation
// semiring with the reward on arcs (log w_a + yh_t(pdf_a)), start states (log pi) and leaks (log c pi).  The logarithms of w
// and pi are doubles made once on the host (den_entropy_tables); terms with pi(h) = 0 or c = 0 are skipped, no log 0 is formed.
//
// In Kaldi's scaling, f_t(a) = w_a exp(yh_t(pdf_a)) / asum_t, r_t(a) = log w_a + yh_t(pdf_a) - k_t, l(h) = log(c pi(h)):
//   forward :  alpha_0 = pi, A_0 = pi log pi;   asum_t = sum_h alpha_t(h);   d_t = sum_h A_t(h) / asum_t
//              alpha'_t = alpha_t + c pi asum_t
//              A'_t(h) = A_t(h) - d_t alpha_t(h) + c pi(h) [sum_g (A_t(g) - d_t alpha_t(g)) + asum_t l(h)]
//              alpha_{t+1}(g) = sum_{a: h->g} alpha'_t(h) f_t(a);   A_{t+1}(g) = sum_{a: h->g} [A'_t(h) + alpha'_t(h) r_t(a)] f_t(a)
//              Z = sum_h alpha'_T(h);   log Z_s = log Z + sum_{t<T} log asum_t;   E~ = sum_h A'_T(h) / Z
//              E[log W] = K + E~,   K = sum_{t<=T} d_t + sum_{t<T} k_t   (in double)
//   backward:  beta'_T = 1 / Z, B'_T = 0;
//              beta_t = beta'_t + c sum_h pi(h) beta'_t(h);   B_t = B'_t + c sum_h pi(h) [B'_t(h) + l(h) beta'_t(h)]
//              beta'_t(h) = sum_{a: h->g} f_t(a) beta_{t+1}(g);   B'_t(h) = sum_{a: h->g} f_t(a) [B_{t+1}(g) + r_t(a) beta_{t+1}(g)]
//   gradient:  dH/dyh_t(j) = -Cov(log W, [the path emits j at t])
//                = - sum_{a: h->g of pdf j} f_t(a) [A'_t(h) beta_{t+1}(g) + alpha'_t(h) ((r_t(a) - E~) beta_{t+1}(g) + B_{t+1}(g))]
// The derivative is taken with respect to the CLAMPED output: an element outside +-kOutputLimit gets the same expression
// (the clamp's own zero derivative is not applied), as in tc_den_expected_accuracy_grad.
//
// Centring.  A_t is the alpha-weighted log-weight of the prefix less the constants subtracted so far; the gradient does not
// depend on them, the arithmetic does.  Here they come from the forward pass itself: d_t makes sum_h (A_t - d_t alpha_t) = 0
// at every level -- the prefix's log-weight is centred on its mean under the forward (filtering) distribution, from the two
// sums the walk forms anyway -- and k_t, which has to be known before frame t's walk, is frame t - 1's whole constant
// k_{t-1} + d_t (k_0 = 0): a guess whose error d_{t+1} then takes out.  The backward pass reads the frames' constants
// k_t + d_{t+1} back as doubles.  So A, B and E~ are of the size of the deviations of log W, not of log W.  Measured against
// float64 on the MI355X (profiles/den_entropy/README.md; the figure is max |got - ref| / max |ref|), 37 states, two sequences
// of 150 frames sharpened along one path so that H = 6.6 beside E[log W] = -1661: entropy 1.3e-7 and gradient 1.9e-5 in this
// form, 1.0e-4 and 2.8e-2 in the uncentred one (d_t = k_t = 0, compiled with -DTC_DEN_ENTROPY_UNCENTRED).  At 7 frames the
// gradient is within 1.9e-6 over the tests' graphs.
//
// Arithmetic.  Every vector by state is float32 where it is stored; every sum over arcs or states is accumulated in double
// and rounded once when it is stored.  The arc factor is the float32 product w * (exp(yh) * (1 / asum)), re-formed per arc.
//
// One workgroup of 16 wavefronts owns one sequence, one launch does everything:
//   scan    : every y of the sequence's valid frames is looked at; a NaN or +-inf gives NaN in entropy and logprob and +0
//             in every gradient row of the sequence.  Padding frames are not read and get +0.
//   forward : frame by frame, lane = destination state walks its in-arcs in the tables' order.  GRAD = false stops here:
//             the value costs a forward pass and no history.  With GRAD alpha'_t and A'_t of every frame go to the
//             workspace, 1 / asum_t and the frame's constant beside them.
//   backward: frame by frame from the last, lane = pdf walks the arcs of its pdf and stores the gradient's element (one store
//             per element, a pdf without arcs gets +0), then lane = source state walks its out-arcs.
// A row of more than kLongRow arcs is walked by its whole wave, lanes striding over the list, and reduced with the xor
// butterfly.  Sums over the states go through a wave butterfly and then the 16 wave sums in wave order.  State h is thread
// h % 1024's in every loop.  The orders are fixed and nothing is atomic: a sequence's bits do not depend on the call, on its
// place in the batch or on the other sequences.
//
// LDS budget (RESIDENT).  Four vectors by state and ONE by pdf, 16 * Hs + 4 * Ps + 1024 <= 163840 bytes, which C3's 8192
// states and 4096 pdfs meet (148480):
//   forward : (alpha_t, A_t) and (alpha'_t, A'_t);
//   backward: X = (beta_{t+1}, B_{t+1}) and Y = (alpha'_t, A'_t) brought back from the workspace.  The by-pdf pass gathers all
//             four; its own yh_t(j) and exp(yh) / asum are the lane's.  The by-source pass gathers X alone and writes beta'_t,
//             B'_t over Y, which is dead by then; X and Y change places.
//   by pdf  : the clamped yh_t, staged once a frame; both the factor and the reward are formed from it per arc.
// Otherwise the vectors are in the workspace, through the same code: the same operations in the same order on the same
// float32 values, so the two forms give the same bits.
#include <float.h>
#include <math.h>

#include "chain_internal.h"

namespace tc {

namespace {

constexpr int kEntThreads = 1024;
constexpr int kEntWaves = kEntThreads / 64;
constexpr int kLongRow = 128;  // arcs beyond which a row is walked by its whole wave

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sums of a and b over the workgroup, in every thread: wave butterflies, then the wave sums in wave order.  Both
// barriers are the caller's too: what was stored before the call is visible after it.
__device__ __forceinline__ void block_sum2(double &a, double &b, double *red, int lane, int wave) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();  // (the slots' readers of the call before)
  if (lane == 0) {
    red[wave] = a;
    red[kEntWaves + wave] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
#pragma unroll
  for (int w = 0; w < kEntWaves; ++w) {
    a += red[w];
    b += red[kEntWaves + w];
  }
}

// Rows r = 0 .. n - 1 of a CSR, lane = row: term(i, r, acc) adds arc i of row r into acc[N], done(r, acc) takes the row's
// sums.  Wave-uniform control around the shuffles: every lane of a wave runs the loop the same number of times.
template <int N, typename Term, typename Done>
__device__ __forceinline__ void walk_rows(const int32_t *begin, int n, int lane, int wave, Term term, Done done) {
  for (int base = wave * 64; base < n; base += kEntThreads) {
    const int r = base + lane;
    int b = 0, e = 0;
    if (r < n) {
      b = begin[r];
      e = begin[r + 1];
    }
    const bool long_row = e - b > kLongRow;
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if (!long_row)
      for (int i = b; i < e; ++i) term(i, r, acc);
    unsigned long long todo = __ballot(long_row);
    while (todo) {
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
      double w[N];
#pragma unroll
      for (int k = 0; k < N; ++k) w[k] = 0.0;
      for (int i = bb + lane; i < ee; i += 64) term(i, base + l, w);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        w[k] = wave_sum(w[k]);
        if (lane == l) acc[k] = w[k];
      }
    }
    if (r < n) done(r, acc);
  }
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

// whether any y of the sequence's T valid frames is a NaN or an infinity (every thread gets the answer): the accuracy
// kernel's scan.  slot: kEntWaves ints of LDS that the next user puts a barrier in front of.
__device__ __forceinline__ bool scan_bad(const float *y, int64_t y_stride, int S, int P, int q, int T, int lane, int wave,
                                         int *slot) {
  int bad = 0;
  for (int t = wave; t < T; t += kEntWaves) {
    const float *row = y + ((int64_t)t * S + q) * y_stride;
    for (int c = lane; c < P; c += 64) bad |= !finite(row[c]);
  }
  const int any = __ballot(bad != 0) != 0;
  if (lane == 0) slot[wave] = any;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < kEntWaves; ++w) all |= slot[w];
  return all != 0;
}

}  // namespace

template <bool RAGGED, bool RESIDENT, bool GRAD>
__global__ __launch_bounds__(kEntThreads) void den_entropy_kernel(const DenEntParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *red = reinterpret_cast<double *>(lds_raw);  // [2][kEntWaves]

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int H = p.H, P = p.P, S = p.S, Hs = p.Hs;

  // ---- scan; the rows nobody computes ----
  const bool bad = scan_bad(p.y, p.y_stride, S, P, q, T, lane, wave, reinterpret_cast<int *>(red));
  if (GRAD)
    for (int t = (bad ? 0 : T) + wave; t < p.T; t += kEntWaves) {
      float *row = p.grad + ((int64_t)t * S + q) * p.grad_stride;
      for (int c = lane; c < P; c += 64) row[c] = 0.0f;
    }
  if (bad) {
    if (tid == 0) {
      p.entropy[q] = NAN;
      p.logprob[q] = NAN;
    }
    return;
  }

  float *seq = reinterpret_cast<float *>(p.workspace) + (int64_t)q * den_ent_seq_floats(H, P, p.T, GRAD);
  double *kk = reinterpret_cast<double *>(seq);  // [T]: the frames' constants (GRAD)
  float *hist_a = seq + 2 * den_acc_round4(p.T + 1), *hist_A = hist_a + (int64_t)(p.T + 1) * Hs;
  float *inv = hist_A + (int64_t)(p.T + 1) * Hs;
  float *ws_vec = GRAD ? inv + den_acc_round4(p.T + 1) : seq;
  float *vec = RESIDENT ? reinterpret_cast<float *>(lds_raw + kDenEntSmallLds) : ws_vec;
  float *v0 = vec, *v1 = vec + Hs, *v2 = vec + 2 * Hs, *v3 = vec + 3 * Hs, *yh = vec + 4 * Hs;
  const float *pi = p.t.t.pi;
  const double *lpi = p.t.log_pi;
  const double c = (double)p.leaky, logc = p.log_leaky;

  // the clamped outputs of frame t, by pdf
  auto stage = [&](int t) {
    const float *yrow = p.y + ((int64_t)t * S + q) * p.y_stride;
    for (int j = tid; j < P; j += kEntThreads) yh[j] = fminf(fmaxf(yrow[j], -kOutputLimit), kOutputLimit);
  };

  // ---- forward: v0, v1 = alpha_t, A_t; v2, v3 = alpha'_t, A'_t ----
  double sa = 0.0, sA = 0.0;
  for (int h = tid; h < H; h += kEntThreads) {
    const float ph = pi[h];
    const float A0 = ph > 0.0f ? (float)((double)ph * lpi[h]) : 0.0f;
    v0[h] = ph;
    v1[h] = A0;
    sa += (double)ph;
    sA += (double)A0;
  }
  block_sum2(sa, sA, red, lane, wave);
  double Z = 0.0, Et = 0.0, K = 0.0, lp = 0.0, khat = 0.0;
  for (int t = 0; t <= T; ++t) {
#ifdef TC_DEN_ENTROPY_UNCENTRED
    const double d = 0.0;
#else
    const double d = sA / sa;
#endif
    K += d;
    if (t > 0) {  // frame t - 1's whole constant: the backward pass's, and the guess for frame t
      khat += d;
      if (GRAD && tid == 0) kk[t - 1] = khat;
#ifdef TC_DEN_ENTROPY_UNCENTRED
      khat = 0.0;
#endif
    }
    const double ca = c * sa, cA = c * (sA - d * sa);
    float *ra = hist_a + (int64_t)t * Hs, *rA = hist_A + (int64_t)t * Hs;
    double za = 0.0, zA = 0.0;
    for (int h = tid; h < H; h += kEntThreads) {
      const double al = (double)v0[h], ph = (double)pi[h];
      double An = (double)v1[h] - d * al;
      if (ph > 0.0 && c > 0.0) An += ph * (cA + ca * (logc + lpi[h]));
      const float ad = (float)(al + ph * ca), Ad = (float)An;
      if (GRAD) {
        ra[h] = ad;
        rA[h] = Ad;
      }
      v2[h] = ad;
      v3[h] = Ad;
      za += (double)ad;
      zA += (double)Ad;
    }
    if (t == T) {
      block_sum2(za, zA, red, lane, wave);
      Z = za;
      Et = zA / za;
      break;
    }
    const float inv_t = (float)(1.0 / sa);
    if (GRAD && tid == 0) inv[t] = inv_t;
    lp += log(sa);
    K += khat;
    stage(t);
    __syncthreads();
    sa = 0.0;
    sA = 0.0;
    walk_rows<2>(
        p.t.t.in_begin, H, lane, wave,
        [&](int i, int, double *acc) {
          const DenAccArc a = p.t.t.in_arcs[i];
          const float yv = yh[a.pdf];
          const double f = (double)(a.w * (expf(yv) * inv_t));
          const double al = (double)v2[a.other];
          acc[0] += al * f;
          acc[1] += ((double)v3[a.other] + al * (p.t.in_logw[i] + (double)yv - khat)) * f;
        },
        [&](int g, const double *acc) {
          const float na = (float)acc[0], nA = (float)acc[1];
          v0[g] = na;
          v1[g] = nA;
          sa += (double)na;
          sA += (double)nA;
        });
    block_sum2(sa, sA, red, lane, wave);
  }
  if (tid == 0) {
    const double logz = lp + log(Z);
    p.logprob[q] = logz;
    p.entropy[q] = logz - (K + Et);
  }
  if (!GRAD) return;

  // ---- backward: X = (beta_{t+1}, B_{t+1}); Y = (alpha'_t, A'_t), then (beta'_t, B'_t), then (beta_t, B_t) ----
  const float scale = p.seq_scale ? p.seq_scale[q] : 1.0f;
  float *x0 = v0, *x1 = v1, *y0 = v2, *y1 = v3;
  {
    const float bT = (float)(1.0 / Z);
    double sb = 0.0, sB = 0.0;
    for (int h = tid; h < H; h += kEntThreads) {
      const double ph = (double)pi[h];
      sb += ph * (double)bT;
      if (ph > 0.0 && c > 0.0) sB += ph * ((logc + lpi[h]) * (double)bT);
    }
    block_sum2(sb, sB, red, lane, wave);  // (its first barrier: the forward pass is done with v0 .. v3)
    const float b = (float)((double)bT + c * sb), B = (float)(c * sB);
    for (int h = tid; h < H; h += kEntThreads) {
      x0[h] = b;
      x1[h] = B;
    }
  }
  for (int t = T - 1; t >= 0; --t) {
    const float inv_t = inv[t];
    const double kt = kk[t];
    stage(t);
    const float *ra = hist_a + (int64_t)t * Hs, *rA = hist_A + (int64_t)t * Hs;
    for (int h = tid; h < H; h += kEntThreads) {
      y0[h] = ra[h];
      y1[h] = rA[h];
    }
    __syncthreads();  // (yh, Y and X of frame t + 1; the first time also the forward pass's history rows)
    float *grow = p.grad + ((int64_t)t * S + q) * p.grad_stride;
    walk_rows<1>(
        p.t.t.pdf_begin, P, lane, wave,
        [&](int i, int j, double *acc) {
          const DenAccPdfArc a = p.t.t.pdf_arcs[i];
          const double b1 = (double)x0[a.dst], al = (double)y0[a.src];
          const double r = p.t.pdf_logw[i] + (double)yh[j] - kt - Et;
          acc[0] += (double)a.w * ((double)y1[a.src] * b1 + al * (r * b1 + (double)x1[a.dst]));
        },
        [&](int j, const double *acc) {
          const float pe = expf(yh[j]) * inv_t;
          grow[j] = 0.0f - scale * (float)((double)pe * acc[0]);  // (0 - x: +0 for a pdf without arcs, whatever the scale's sign)
        });
    if (t == 0) break;
    __syncthreads();  // (the by-pdf pass is done with Y)
    double sb = 0.0, sB = 0.0;
    walk_rows<2>(
        p.t.t.out_begin, H, lane, wave,
        [&](int i, int, double *acc) {
          const DenAccArc a = p.t.t.out_arcs[i];
          const float yv = yh[a.pdf];
          const double f = (double)(a.w * (expf(yv) * inv_t));
          const double b1 = (double)x0[a.other];
          acc[0] += f * b1;
          acc[1] += f * ((double)x1[a.other] + (p.t.out_logw[i] + (double)yv - kt) * b1);
        },
        [&](int h, const double *acc) {
          const float b = (float)acc[0], B = (float)acc[1];
          y0[h] = b;
          y1[h] = B;
          const double ph = (double)pi[h];
          sb += ph * (double)b;
          if (ph > 0.0 && c > 0.0) sB += ph * ((double)B + (logc + lpi[h]) * (double)b);
        });
    block_sum2(sb, sB, red, lane, wave);
    const double lb = c * sb, lB = c * sB;
    for (int h = tid; h < H; h += kEntThreads) {  // (a state's own thread: the one that stored beta'_t(h) above)
      y0[h] = (float)((double)y0[h] + lb);
      y1[h] = (float)((double)y1[h] + lB);
    }
    float *x = x0;
    x0 = y0;
    y0 = x;
    x = x1;
    x1 = y1;
    y1 = x;
  }
}

namespace {

template <bool RAGGED, bool RESIDENT, bool GRAD>
int launch_form(const DenEntParams &p, hipStream_t stream) {
  void (*kernel)(const DenEntParams) = den_entropy_kernel<RAGGED, RESIDENT, GRAD>;
  const size_t lds = kDenEntSmallLds + (RESIDENT ? (size_t)4 * den_ent_frame_floats(p.H, p.P) : 0);
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kEntThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <bool RAGGED, bool RESIDENT>
int launch_grad(const DenEntParams &p, hipStream_t stream) {
  return p.grad ? launch_form<RAGGED, RESIDENT, true>(p, stream) : launch_form<RAGGED, RESIDENT, false>(p, stream);
}

}  // namespace

int launch_den_entropy(const DenEntParams &p, hipStream_t stream) {
  if (!p.y || !p.entropy || !p.logprob || !p.workspace || !p.t.t.in_arcs || !p.t.in_logw) return TC_ERR_INVALID_ARGUMENT;
  if (p.resident && !den_ent_resident(p.H, p.P)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenEntropy);
  if (!p.resident) count_launch(kCntDenEntropyStreamed);
  if (p.seq_frames) return p.resident ? launch_grad<true, true>(p, stream) : launch_grad<true, false>(p, stream);
  return p.resident ? launch_grad<false, true>(p, stream) : launch_grad<false, false>(p, stream);
}

}  // namespace tc
