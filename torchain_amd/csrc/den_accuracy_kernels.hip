// Expected frame accuracy over the denominator graph and its gradient, for gfx950 (tc_den_expected_accuracy,
// tc_den_expected_accuracy_grad): the lattice-free sMBR criterion (Kanda et al. 2018) on den.fst.
//
//     E_s[A] = sum_paths P(path | y_s) * sum_t a_t(pdf_t(path)),      a_t(j) = [0 <= ref_t < P and class(j) == class(ref_t)]
//
// with the denominator's own model: p_t(j) = exp(clamp(y_t(j), +-kOutputLimit)), the graph's initial probabilities pi, the
// leaky-HMM coefficient c, every state final.  DENSE (tc_den_expected_accuracy_dense, _dense_grad): a_t(j) is not that
// indicator but element j of row t*S + s of a float32 matrix the caller gives -- the numerator's posteriors (Kaldi's
// chain-sMBR), label-smoothed indicators, signed rewards: any finite float32.  Only the places that produce a_t(j) differ
// (the row kernel's m_t, stage() below, and the scan, which looks at the sequence's valid rows of the matrix beside y's);
// the recursions and the centring argument do not depend on what a_t(j) is, and the hard form's instantiations are the
// instruction streams they were (profiles/den_accuracy_dense/kernel_isa.txt).
//
// The value needs nothing new: m_t = sum_j gamma_t(j) a_t(j) from the denominator posteriors the tuned kernels write, and
// E_s = sum_t m_t (den_accuracy_rows_kernel, one workgroup per sequence, the frames in order, in double).
//
// The gradient needs a second forward-backward that carries the accuracy (den_accuracy_grad_kernel).  In Kaldi's scaling,
// with at_t(j) = a_t(j) - m_t and f_t(arc) = w * p_t(pdf) / asum_t:
//   forward :  alpha_0 = pi, A_0 = 0;   asum_t = sum_h alpha_t(h);
//              alpha'_t = alpha_t + c pi asum_t;                 A'_t = A_t + c pi sum_h A_t(h)
//              alpha_{t+1}(g) = sum_{h->g} alpha'_t(h) f_t;      A_{t+1}(g) = sum_{h->g} [A'_t(h) + alpha'_t(h) at_t(pdf)] f_t
//              Z = sum_h alpha'_T(h);                            E~ = sum_h A'_T(h) / Z
//   backward:  beta'_T = 1 / Z, B'_T = 0;
//              beta_t = beta'_t + c sum_h pi(h) beta'_t(h);      B_t = B'_t + c sum_h pi(h) B'_t(h)
//              beta'_t(h) = sum_{h->g} f_t beta_{t+1}(g);        B'_t(h) = sum_{h->g} f_t [B_{t+1}(g) + at_t(pdf) beta_{t+1}(g)]
//   gradient:  dE/dy_t(j) = sum_{arcs h->g of pdf j} f_t [A'_t(h) beta_{t+1}(g) + alpha'_t(h) (at_t(j) beta_{t+1}(g) + B_{t+1}(g)
//                                                                                            - beta_{t+1}(g) E~)]
// The gradient does not depend on the per-frame constants m_t subtracted from a_t; the arithmetic does.  Uncentred, A, B and
// E~ are of the size of E[A] and the gradient is their small difference; centred with the frame's expected accuracy they are
// of the size of the deviations, E~ is a rounding residue, and float32 vectors carry the gradient to a few 1e-7 of its
// largest element where the uncentred form loses three digits (profiles/den_accuracy/README.md).
//
// Arithmetic.  Every vector -- alpha, A, alpha', A', beta, B by state, exp(y) / asum and at by pdf -- is float32 where it
// is stored; every sum over arcs or states is accumulated in double and rounded once when it is stored.  The arc factor is
// the float32 product w * (exp(y) / asum).
//
// One workgroup of 16 wavefronts owns one sequence, one launch does everything:
//   scan    : every y of the sequence's valid frames is looked at; a NaN or +-inf gives +0 in every row of the sequence.
//   forward : frame by frame, lane = destination state walks its in-arcs in the tables' order; alpha'_t and A'_t of every
//             frame go to the workspace, 1 / asum_t beside them.
//   backward: frame by frame from the last, lane = pdf walks the arcs of its pdf and stores the gradient's element (one
//             store per element, a pdf without arcs gets +0), then lane = source state walks its out-arcs.
// A row of more than kLongRow arcs (a state's or a pdf's) is walked by its whole wave, lanes striding over the list, and
// reduced with a butterfly: x + y is commutative, so the 64 lanes end with the same bits.  Sums over the states go through
// a wave butterfly and then the 16 wave sums in wave order.  The orders are fixed and nothing is atomic: a sequence's bits
// do not depend on the call, on its place in the batch or on the other sequences.
// RESIDENT: the per-frame vectors (four by state, two by pdf) are in LDS; otherwise they are in the workspace, through the
// same code -- the same operations in the same order on the same float32 values, so the two forms give the same bits.
#include <float.h>
#include <math.h>

#include "chain_internal.h"

namespace tc {

namespace {

constexpr int kAccThreads = 1024;
constexpr int kAccWaves = kAccThreads / 64;
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
    red[kAccWaves + wave] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
#pragma unroll
  for (int w = 0; w < kAccWaves; ++w) {
    a += red[w];
    b += red[kAccWaves + w];
  }
}

// Rows r = 0 .. n - 1 of a CSR, lane = row: term(i, r, acc) adds arc i of row r into acc[N], done(r, acc) takes the row's
// sums.  Wave-uniform control around the shuffles: every lane of a wave runs the loop the same number of times.
template <int N, typename Term, typename Done>
__device__ __forceinline__ void walk_rows(const int32_t *begin, int n, int lane, int wave, Term term, Done done) {
  for (int base = wave * 64; base < n; base += kAccThreads) {
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

// whether any y of the sequence's T valid frames is a NaN or an infinity (every thread gets the answer).  slot: kAccWaves
// ints of LDS that the next user puts a barrier in front of.  (Not __syncthreads_or: it brings static LDS with it, which
// comes off what the gradient kernel may ask for and moves the base of its dynamic region.)  DENSE: or any a of the same
// rows of the accuracy matrix; its padding rows are not read either.
template <bool DENSE>
__device__ __forceinline__ bool scan_bad(const float *y, int64_t y_stride, const float *a, int64_t a_stride, int S, int P, int q,
                                         int T, int lane, int wave, int *slot) {
  int bad = 0;
  for (int t = wave; t < T; t += kAccWaves) {
    const float *row = y + ((int64_t)t * S + q) * y_stride;
    for (int c = lane; c < P; c += 64) bad |= !finite(row[c]);
    if (DENSE) {
      const float *arow = a + ((int64_t)t * S + q) * a_stride;
      for (int c = lane; c < P; c += 64) bad |= !finite(arow[c]);
    }
  }
  const int any = __ballot(bad != 0) != 0;
  if (lane == 0) slot[wave] = any;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < kAccWaves; ++w) all |= slot[w];
  return all != 0;
}

// a_t(j) of a frame whose reference is r
__device__ __forceinline__ bool ref_ok(int r, int P) { return r >= 0 && r < P; }
__device__ __forceinline__ int class_of(const int32_t *pdf_class, int j) { return pdf_class ? pdf_class[j] : j; }

}  // namespace

template <bool DENSE>
__global__ __launch_bounds__(kAccThreads) void den_accuracy_rows_kernel(const DenAccRowParams p) {
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.seq_frames ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  __shared__ int slot[kAccWaves];
  const bool bad = scan_bad<DENSE>(p.y, p.y_stride, p.accuracy, p.acc_stride, p.S, p.P, q, T, lane, wave, slot);
  float *fa = p.frame_acc + (int64_t)q * p.T;
  for (int t = wave; t < p.T; t += kAccWaves) {
    double m = 0.0;
    if (t < T && !bad) {
      if (DENSE) {  // (an indicator's products are g * 1 and g * 0, exact fused or not: the hard form's sum)
        const float *g = p.gamma + ((int64_t)t * p.S + q) * p.gamma_stride;
        const float *a = p.accuracy + ((int64_t)t * p.S + q) * p.acc_stride;
        for (int j = lane; j < p.P; j += 64) m += (double)g[j] * (double)a[j];
      } else {
        const int r = p.ref[(int64_t)q * p.T + t];
        if (ref_ok(r, p.P)) {  // (wave-uniform)
          const int cr = class_of(p.pdf_class, r);
          const float *g = p.gamma + ((int64_t)t * p.S + q) * p.gamma_stride;
          for (int j = lane; j < p.P; j += 64)
            if (class_of(p.pdf_class, j) == cr) m += (double)g[j];
        }
      }
      m = wave_sum(m);
    }
    if (lane == 0) fa[t] = (t < T && bad) ? NAN : (float)m;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
    for (int t = 0; t < T; ++t) e += (double)fa[t];
    p.acc[q] = e;  // (NaN when the sequence is not finite: its frames are)
  }
}

template <bool RAGGED, bool RESIDENT, bool DENSE>
__global__ __launch_bounds__(kAccThreads) void den_accuracy_grad_kernel(const DenAccGradParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *red = reinterpret_cast<double *>(lds_raw);  // [2][kAccWaves]

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int H = p.H, P = p.P, S = p.S, Hs = p.Hs;
  const float scale = p.seq_scale ? p.seq_scale[q] : 1.0f;

  // ---- scan; the rows nobody computes ----
  const bool bad = scan_bad<DENSE>(p.y, p.y_stride, p.accuracy, p.acc_stride, S, P, q, T, lane, wave, reinterpret_cast<int *>(red));
  for (int t = (bad ? 0 : T) + wave; t < p.T; t += kAccWaves) {
    float *row = p.grad + ((int64_t)t * S + q) * p.grad_stride;
    for (int c = lane; c < P; c += 64) row[c] = 0.0f;
  }
  if (bad) return;

  float *seq = reinterpret_cast<float *>(p.workspace) + (int64_t)q * den_acc_seq_floats(H, P, p.T);
  float *hist_a = seq, *hist_A = seq + (int64_t)(p.T + 1) * Hs;
  float *inv = hist_A + (int64_t)(p.T + 1) * Hs;
  float *vec = RESIDENT ? reinterpret_cast<float *>(lds_raw + kDenAccSmallLds) : inv + den_acc_round4(p.T + 1);
  float *v0 = vec, *v1 = vec + Hs, *v2 = vec + 2 * Hs, *v3 = vec + 3 * Hs;
  float *pe = vec + 4 * Hs, *at = pe + p.Ps;
  const float *pi = p.t.pi;
  const double c = (double)p.leaky;

  // exp(y_t) / asum_t and the centred accuracies of frame t, by pdf (the same expressions in both passes)
  auto stage = [&](int t, float inv_t) {
    const float *yrow = p.y + ((int64_t)t * S + q) * p.y_stride;
    if (DENSE) {  // (the dense row is read where y's is)
      const float *arow = p.accuracy + ((int64_t)t * S + q) * p.acc_stride;
      const float m = p.frame_acc[(int64_t)q * p.T + t];
      for (int j = tid; j < P; j += kAccThreads) {
        const float yc = fminf(fmaxf(yrow[j], -kOutputLimit), kOutputLimit);
        pe[j] = expf(yc) * inv_t;
        at[j] = arow[j] - m;
      }
      return;
    }
    const int r = p.ref[(int64_t)q * p.T + t];
    const bool ok = ref_ok(r, P);
    const int cr = ok ? class_of(p.pdf_class, r) : 0;
    const float m = p.frame_acc[(int64_t)q * p.T + t];
    for (int j = tid; j < P; j += kAccThreads) {
      const float yc = fminf(fmaxf(yrow[j], -kOutputLimit), kOutputLimit);
      pe[j] = expf(yc) * inv_t;
      at[j] = ((ok && class_of(p.pdf_class, j) == cr) ? 1.0f : 0.0f) - m;
    }
  };

  // ---- forward: v0, v1 = alpha_t, A_t; v2, v3 = alpha'_t, A'_t ----
  double sa = 0.0, sA = 0.0;
  for (int h = tid; h < H; h += kAccThreads) {
    v0[h] = pi[h];
    v1[h] = 0.0f;
    sa += (double)pi[h];
  }
  block_sum2(sa, sA, red, lane, wave);
  double Z = 0.0, Et = 0.0;
  for (int t = 0; t <= T; ++t) {
    const double ca = c * sa, cA = c * sA;
    float *ra = hist_a + (int64_t)t * Hs, *rA = hist_A + (int64_t)t * Hs;
    double za = 0.0, zA = 0.0;
    for (int h = tid; h < H; h += kAccThreads) {
      const float ad = (float)((double)v0[h] + (double)pi[h] * ca);
      const float Ad = (float)((double)v1[h] + (double)pi[h] * cA);
      ra[h] = ad;
      rA[h] = Ad;
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
    if (tid == 0) inv[t] = inv_t;
    stage(t, inv_t);
    __syncthreads();
    sa = 0.0;
    sA = 0.0;
    walk_rows<2>(
        p.t.in_begin, H, lane, wave,
        [&](int i, int, double *acc) {
          const DenAccArc a = p.t.in_arcs[i];
          const double f = (double)(a.w * pe[a.pdf]);
          const double al = (double)v2[a.other];
          acc[0] += al * f;
          acc[1] += ((double)v3[a.other] + al * (double)at[a.pdf]) * f;
        },
        [&](int h, const double *acc) {
          const float na = (float)acc[0], nA = (float)acc[1];
          v0[h] = na;
          v1[h] = nA;
          sa += (double)na;
          sA += (double)nA;
        });
    block_sum2(sa, sA, red, lane, wave);
  }

  // ---- backward: (cb, cB) = beta_{t+1}, B_{t+1}; (nb, nB) receive beta_t, B_t ----
  float *cb = v0, *cB = v1, *nb = v2, *nB = v3;
  {
    const float bT = (float)(1.0 / Z);
    double sb = 0.0, sB = 0.0;
    for (int h = tid; h < H; h += kAccThreads) sb += (double)pi[h] * (double)bT;
    block_sum2(sb, sB, red, lane, wave);  // (its first barrier: the forward pass is done with v0 .. v3)
    const float b = (float)((double)bT + c * sb);
    for (int h = tid; h < H; h += kAccThreads) {
      cb[h] = b;
      cB[h] = 0.0f;
    }
  }
  for (int t = T - 1; t >= 0; --t) {
    stage(t, inv[t]);
    __syncthreads();  // (pe, at and the vectors of frame t + 1; the first time also the forward pass's history rows)
    const float *ra = hist_a + (int64_t)t * Hs, *rA = hist_A + (int64_t)t * Hs;
    float *grow = p.grad + ((int64_t)t * S + q) * p.grad_stride;
    walk_rows<1>(
        p.t.pdf_begin, P, lane, wave,
        [&](int i, int j, double *acc) {
          const DenAccPdfArc a = p.t.pdf_arcs[i];
          const double b1 = (double)cb[a.dst], al = (double)ra[a.src];
          acc[0] += (double)a.w * ((double)rA[a.src] * b1 + al * ((double)at[j] * b1 + (double)cB[a.dst] - b1 * Et));
        },
        [&](int j, const double *acc) { grow[j] = scale * (float)((double)pe[j] * acc[0]); });
    if (t == 0) break;
    double sb = 0.0, sB = 0.0;
    walk_rows<2>(
        p.t.out_begin, H, lane, wave,
        [&](int i, int, double *acc) {
          const DenAccArc a = p.t.out_arcs[i];
          const double f = (double)(a.w * pe[a.pdf]);
          const double b1 = (double)cb[a.other];
          acc[0] += f * b1;
          acc[1] += f * ((double)cB[a.other] + (double)at[a.pdf] * b1);
        },
        [&](int h, const double *acc) {
          const float b = (float)acc[0], B = (float)acc[1];
          nb[h] = b;
          nB[h] = B;
          sb += (double)pi[h] * (double)b;
          sB += (double)pi[h] * (double)B;
        });
    block_sum2(sb, sB, red, lane, wave);
    const double lb = c * sb, lB = c * sB;
    for (int h = tid; h < H; h += kAccThreads) {  // (a state's own thread: the one that stored beta'_t(h) above)
      nb[h] = (float)((double)nb[h] + lb);
      nB[h] = (float)((double)nB[h] + lB);
    }
    float *x = cb;
    cb = nb;
    nb = x;
    x = cB;
    cB = nB;
    nB = x;
  }
}

namespace {

template <bool RAGGED, bool RESIDENT, bool DENSE>
int launch_grad(const DenAccGradParams &p, hipStream_t stream) {
  void (*kernel)(const DenAccGradParams) = den_accuracy_grad_kernel<RAGGED, RESIDENT, DENSE>;
  const size_t lds = kDenAccSmallLds + (RESIDENT ? (size_t)4 * den_acc_frame_floats(p.H, p.P) : 0);
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kAccThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <bool DENSE>
int launch_grad_form(const DenAccGradParams &p, hipStream_t stream) {
  if (p.seq_frames) return p.resident ? launch_grad<true, true, DENSE>(p, stream) : launch_grad<true, false, DENSE>(p, stream);
  return p.resident ? launch_grad<false, true, DENSE>(p, stream) : launch_grad<false, false, DENSE>(p, stream);
}

}  // namespace

// dense: p.accuracy and p.acc_stride are set, not p.ref and p.pdf_class
int launch_den_accuracy_rows(const DenAccRowParams &p, bool dense, hipStream_t stream) {
  if (!p.y || !p.gamma || !p.ref || !p.frame_acc || !p.acc) return TC_ERR_INVALID_ARGUMENT;  // (ref: or accuracy)
  if (dense && p.acc_stride < p.P) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenAccuracy);
  if (dense) {
    count_launch(kCntDenAccuracyDense);
    hipLaunchKernelGGL(den_accuracy_rows_kernel<true>, dim3(p.S), dim3(kAccThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL(den_accuracy_rows_kernel<false>, dim3(p.S), dim3(kAccThreads), 0, stream, p);
  }
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_den_accuracy_grad(const DenAccGradParams &p, bool dense, hipStream_t stream) {
  if (!p.y || !p.ref || !p.frame_acc || !p.grad || !p.workspace || !p.t.in_arcs) return TC_ERR_INVALID_ARGUMENT;
  if (dense && p.acc_stride < p.P) return TC_ERR_INVALID_ARGUMENT;
  if (p.resident && !den_acc_resident(p.H, p.P)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenAccuracyGrad);
  if (!p.resident) count_launch(kCntDenAccuracyGradStreamed);
  if (dense) count_launch(kCntDenAccuracyDenseGrad);
  return dense ? launch_grad_form<true>(p, stream) : launch_grad_form<false>(p, stream);
}

}  // namespace tc
