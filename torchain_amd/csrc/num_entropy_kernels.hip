// Entropy of an end-to-end supervision's path posterior and its gradient, for gfx950 (tc_supervision_path_entropy).
//
// Paths are the sequences of exactly T arcs from the sequence's start state to a final state of its (cyclic) FST, with
// log W(path) = sum_t (y_t(pdf_t) - cost_t) - final cost.  H = log Z - E[log W], and dH / dy_t(j) is minus the covariance of
// log W with "pdf j at frame t".  Both are first-order quantities of the EXPECTATION semiring; here it is carried in the log
// domain and in MEAN form, so that nothing has to be centred: beside log alpha_t(j) a state holds
//   Abar_t(j) = E[log W of the prefix | the prefix ends in j at t],
// which is of the size of log W itself whatever the weights are, and is kept in double:
//   forward : x_a = log alpha_t(i) + r_a, r_a = (y_t(pdf_a) - cost_a), over the in-arcs a: i -> j of state j;
//             log alpha_{t+1}(j) = logsum x_a;  share_a = exp(x_a - max) / sum;  Abar_{t+1}(j) = sum share_a (Abar_t(i) + r_a).
//             log Z = logsum_i log alpha_T(i) - final(i), E[log W] = the same shares' mean of Abar_T(i) - final(i).
//   backward: (log beta_t(i), Bbar_t(i)) over the out-arcs in the same way from log beta_T = Bbar_T = -final;  the arc's term
//             occ_a (Abar_t(i) + r_a + Bbar_{t+1}(dst) - E[log W]),  occ_a = exp(log alpha_t(i) + r_a + log beta_{t+1}(dst) - log Z),
//             goes to one float per arc; each distinct pdf sums its arcs' terms in table order and makes ONE store of
//             -grad_output * sum.
// The log-sum is num_e2e_kernel's, operand for operand (r_a one float32 sum, the float32 exp of a double difference, the
// float32 sum of the shares under a double log), so log Z has the numerator's bits; the means divide a double sum of
// share * value by the double sum of the same shares.
//
// One workgroup of 256 threads owns one sequence.  Threads own states (thread j walks the arc lists of states j, j + 256,
// ...) and distinct pdfs (thread k stages y and sums the terms of pdfs k, k + 256, ...); the first TC_E2E_MAX_PDFS / 256 of a
// thread's pdfs have their y loaded a frame ahead into registers, further ones (handles of tc_supervision_create_e2e_any
// only) are loaded where they are staged.  Two barriers a frame in each direction.
// LDS, laid out with the sequence's own sizes: [2][MS] log alpha | [2][MS] Abar (the backward pass: log beta, Bbar) as
// doubles, [MP] the frame's y, and [arcs] the terms when the handle's largest counts leave them room
// (num_ent_terms_in_lds) -- otherwise the terms live in the caller's workspace and the same statements address them.
// 2048 states, 1024 pdfs and 8192 arcs take 64 + 4 + 32 KB of the 160.
// The history (log alpha_t, Abar_t), t < T, is one 16-byte store a (frame, state) into the CALLER'S workspace: the
// supervision's pool slot is read for its tables alone, so what a training step finds there is what it left.  y is read
// again from the caller's tensor on the way back.  GRAD = false: the forward pass alone, no history.
//
// The gradient buffer is defined everywhere: the workgroup first writes +0 into every element of its sequence -- padding
// frames and pdfs without arcs keep it -- and a failed sequence returns before the backward pass.  Failure: no path of T
// arcs (log Z = -inf: logprob -inf, entropy NaN), or a NaN / +-inf among the y the sequence reads (both NaN; found by the
// threads that stage y, not left to the recursion, where a max would drop a NaN).  No atomics, every sum in a fixed order, and
// nothing depends on blockIdx but the sequence's own data: a sequence's bits do not depend on its batch.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kEntThreads = kE2eThreads;
constexpr int kEntPdfRegs = TC_E2E_MAX_PDFS / kEntThreads;

__device__ __forceinline__ double ent_wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename El>
__device__ __forceinline__ void ent_store(void *g, int64_t i, float v) {
  if constexpr (std::is_same<El, float>::value)
    reinterpret_cast<float *>(g)[i] = v;
  else
    reinterpret_cast<uint16_t *>(g)[i] = Elem<El>::round(v);
}

// element (frame t, pdf) of sequence q of the gradient, laid out as y is
template <typename El>
__device__ __forceinline__ void ent_store_grad(const NumEntParams &p, int q, int t, int pdf, float v) {
  if (p.n.y_bct)
    ent_store<El>(p.grad, ((int64_t)q * p.n.P + pdf) * p.n.T + t, v);
  else
    reinterpret_cast<float *>(p.grad)[((int64_t)t * p.n.S + q) * p.grad_stride + pdf] = v;
}

// One state's step of either recursion over its arc list [b, e): `la`, `ma` are the other level's log weights and means,
// a key's low half the state there and its high half the arc's pdf slot in E.  TERMS (the backward pass): the arc's
// gradient term on the way, from al = log alpha_t(i) - log Z and dv = Abar_t(i) - E[log W] of this state.
template <bool TERMS>
__device__ __forceinline__ void ent_row(int b, int e, const uint32_t *key, const float *lw, const float *E, const double *la,
                                        const double *ma, double *la_out, double *ma_out, double al, double dv, float *term) {
  double mx = -INFINITY;
  for (int a = b; a < e; ++a) {
    const uint32_t k = key[a];
    const int o = (int)(k & 0xffffu);
    const double r = (double)(lw[a] + E[k >> 16]);
    const double x = la[o] + r;
    mx = fmax(mx, x);
    if (TERMS) {
      const float occ = __expf((float)(al + x));  // (exp(-inf) = 0: an arc no path takes)
      term[a] = occ > 0.f ? (float)((double)occ * (dv + r + ma[o])) : 0.f;
    }
  }
  double acc = mx, mean = 0.0;
  if (mx > -INFINITY) {
    float sum = 0.f;
    double num = 0.0, den = 0.0;
    for (int a = b; a < e; ++a) {
      const uint32_t k = key[a];
      const int o = (int)(k & 0xffffu);
      const double r = (double)(lw[a] + E[k >> 16]);
      const float sh = __expf((float)(la[o] + r - mx));
      sum += sh;
      if (sh > 0.f) {  // (a share of 0 may stand before an infinite cost)
        num += (double)sh * (ma[o] + r);
        den += (double)sh;
      }
    }
    acc = mx + log((double)sum);
    mean = num / den;
  }
  *la_out = acc;
  *ma_out = mean;
}

}  // namespace

template <typename El, bool RAGGED, bool GRAD>
__global__ __launch_bounds__(kEntThreads) void num_entropy_kernel(const NumEntParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_x[4], red_n[4], red_d[4];
  __shared__ float red_s[4];
  __shared__ int red_bad[4];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? n.seq_frames[q] : n.T;
  const SeqView v = seq_view(n, q);  // (its hist and stage point into the pool slot: not used here)
  const int MS = (v.n + 3) & ~3, MP = (v.np + 3) & ~3;
  double *LA = reinterpret_cast<double *>(lds_raw);  // [2][MS]: log alpha (forward), log beta (backward)
  double *MA = LA + 2 * MS;                          // [2][MS]: Abar, Bbar
  float *E = reinterpret_cast<float *>(MA + 2 * MS);  // [MP]: the frame's y per distinct pdf
  float *TERM = nullptr;                              // [arcs]: the frame's gradient terms (backward)
  double2 *hist = nullptr;                            // [T][n]: (log alpha_t, Abar_t)
  if (GRAD) {
    TERM = p.terms_in_lds ? E + MP : p.terms + n.t.e2e_tab.arc_off[q];
    hist = reinterpret_cast<double2 *>(p.hist) + (int64_t)n.T * v.sb;
  }
  const int start = n.t.e2e_tab.start[q];

  if (GRAD) {  // +0 everywhere; the backward pass stores over it behind the barriers of the forward pass
    if (n.y_bct) {
      const int64_t base = (int64_t)q * n.P * n.T, cnt = (int64_t)n.P * n.T;
      for (int64_t i = tid; i < cnt; i += kEntThreads) ent_store<El>(p.grad, base + i, 0.f);
    } else {
      float *g = reinterpret_cast<float *>(p.grad);
      for (int t = 0; t < n.T; ++t) {
        float *row = g + ((int64_t)t * n.S + q) * p.grad_stride;
        for (int j = tid; j < n.P; j += kEntThreads) row[j] = 0.f;
      }
    }
  }

  int pk[kEntPdfRegs];  // the first pdfs this thread owns (-1: none)
  float ynx[kEntPdfRegs];
#pragma unroll
  for (int r = 0; r < kEntPdfRegs; ++r) {
    const int k = tid + r * kEntThreads;
    pk[r] = k < v.np ? v.pdf_of[k] : -1;
    ynx[r] = pk[r] >= 0 ? load_y<El>(n, q, 0, pk[r]) : 0.f;
  }
  bool bad = false;
  // frame t's y into E; `ahead` (-1: none) is the frame the registers fetch next
  auto stage_y = [&](int t, int ahead) {
#pragma unroll
    for (int r = 0; r < kEntPdfRegs; ++r) {
      if (pk[r] < 0) continue;
      E[tid + r * kEntThreads] = ynx[r];
      bad |= !(ynx[r] - ynx[r] == 0.f);
      if (ahead >= 0) ynx[r] = load_y<El>(n, q, ahead, pk[r]);
    }
    for (int k = tid + kEntPdfRegs * kEntThreads; k < v.np; k += kEntThreads) {
      const float y = load_y<El>(n, q, t, v.pdf_of[k]);
      E[k] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward ----
  for (int i = tid; i < v.n; i += kEntThreads) {
    LA[i] = i == start ? 0.0 : -INFINITY;
    MA[i] = 0.0;
  }
  int c = 0;
  for (int t = 0; t < T; ++t) {
    stage_y(t, t + 1 < T ? t + 1 : -1);
    __syncthreads();
    const double *a_cur = LA + c * MS, *m_cur = MA + c * MS;
    double *a_nxt = LA + (1 - c) * MS, *m_nxt = MA + (1 - c) * MS;
    for (int j = tid; j < v.n; j += kEntThreads) {
      if (GRAD) hist[(int64_t)t * v.n + j] = make_double2(a_cur[j], m_cur[j]);
      ent_row<false>(v.in_begin[j], v.in_begin[j + 1], v.in_key, v.in_lw, E, a_cur, m_cur, a_nxt + j, m_nxt + j, 0.0, 0.0,
                     nullptr);
    }
    __syncthreads();
    c = 1 - c;
  }

  // log Z and E[log W] over the final states, by fixed-order reductions
  double logz, elw;
  bool any_bad;
  {
    const double *a_T = LA + c * MS, *m_T = MA + c * MS;
    double mx = -INFINITY;
    for (int i = tid; i < v.n; i += kEntThreads) mx = fmax(mx, a_T[i] + (double)v.final_lw[i]);
    mx = e2e_wave_max_d(mx);
    if (lane == 0) red_x[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3]));
    float sum = 0.f;
    double num = 0.0, den = 0.0;
    if (mx > -INFINITY)
      for (int i = tid; i < v.n; i += kEntThreads) {
        const double fl = (double)v.final_lw[i];
        const float sh = __expf((float)(a_T[i] + fl - mx));
        sum += sh;
        if (sh > 0.f) {
          num += (double)sh * (m_T[i] + fl);
          den += (double)sh;
        }
      }
    sum = e2e_wave_sum(sum);
    num = ent_wave_sum_d(num);
    den = ent_wave_sum_d(den);
    const int wbad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      red_s[wave] = sum;
      red_n[wave] = num;
      red_d[wave] = den;
      red_bad[wave] = wbad;
    }
    __syncthreads();
    logz = mx > -INFINITY ? mx + log((double)((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]))) : -INFINITY;
    elw = ((red_n[0] + red_n[1]) + (red_n[2] + red_n[3])) / ((red_d[0] + red_d[1]) + (red_d[2] + red_d[3]));
    any_bad = (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3]) != 0 || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  }
  const bool ok = !any_bad && logz > -INFINITY;
  if (tid == 0) {
    p.logprob[q] = any_bad ? (double)NAN : logz;
    p.entropy[q] = ok ? logz - elw : (double)NAN;
  }
  if (!GRAD || !ok) return;

  // ---- backward, with the gradient ----
  const double scale = p.grad_output ? p.grad_output[q] : 1.0;
  c = 0;
  for (int i = tid; i < v.n; i += kEntThreads) {
    const double fl = (double)v.final_lw[i];
    LA[i] = fl;
    MA[i] = fl > -INFINITY ? fl : 0.0;
  }
  // (the registers hold frame T - 1's y: the forward pass's last fetch)
  for (int t = T - 1; t >= 0; --t) {
    stage_y(t, t > 0 ? t - 1 : -1);
    __syncthreads();
    const double *b_cur = LA + c * MS, *m_cur = MA + c * MS;
    double *b_nxt = LA + (1 - c) * MS, *m_nxt = MA + (1 - c) * MS;
    for (int i = tid; i < v.n; i += kEntThreads) {
      const double2 h = hist[(int64_t)t * v.n + i];
      ent_row<true>(v.out_begin[i], v.out_begin[i + 1], v.out_key, v.out_lw, E, b_cur, m_cur, b_nxt + i, m_nxt + i, h.x - logz,
                    h.y - elw, TERM);
    }
    __syncthreads();
    for (int k = tid; k < v.np; k += kEntThreads) {
      float g = 0.f;
      for (int i = v.pdf_begin[k]; i < v.pdf_begin[k + 1]; ++i) g += TERM[v.pdf_arc[i]];
      ent_store_grad<El>(p, q, t, v.pdf_of[k], (float)(-scale * (double)g));
    }
    c = 1 - c;
  }
}

namespace {

template <typename El, bool RAGGED, bool GRAD>
int launch_ent(const NumEntParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumEntParams) = num_entropy_kernel<El, RAGGED, GRAD>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kEntThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename El>
int launch_ent(const NumEntParams &p, size_t lds, hipStream_t stream) {
  if (p.n.seq_frames) return p.grad ? launch_ent<El, true, true>(p, lds, stream) : launch_ent<El, true, false>(p, lds, stream);
  return p.grad ? launch_ent<El, false, true>(p, lds, stream) : launch_ent<El, false, false>(p, lds, stream);
}

}  // namespace

int launch_num_entropy(const NumEntParams &p, hipStream_t stream) {
  if (!p.n.t.e2e || !p.entropy || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (p.grad && (!p.hist || (!p.terms_in_lds && !p.terms))) return TC_ERR_WORKSPACE;
  const E2eDev &e = p.n.t.e2e_tab;
  // laid out per sequence (the size rule is per sequence): no more than the handle's largest counts side by side, and no
  // more than the rule admits
  size_t lds = num_ent_lds_bytes(e.max_states, p.grad && p.terms_in_lds ? e.max_arcs : 0, e.max_pdfs);
  const size_t rule = (size_t)kLdsLimitBytes - kNumEntStaticLds;
  if (lds > rule) lds = rule;
  count_launch(kCntNumEntropy);
  if (p.n.elem == TC_DTYPE_BF16) return launch_ent<__hip_bfloat16>(p, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_ent<__half>(p, lds, stream);
  return launch_ent<float>(p, lds, stream);
}

}  // namespace tc
