// Numerator of end-to-end supervisions for gfx950: [K] GenericNumeratorComputation (chain-generic-numerator.cc).
//
// Kaldi copies the numerator's rows of nnet_output to the host and runs the forward-backward over each sequence's FST
// (cycles allowed, one arc per frame) in a CPU loop.  Here one workgroup of 256 threads owns one sequence and walks its
// T frames in the log semiring, alpha and beta in double (as num_kernels.hip does):
//   forward : alpha_{t+1}(j) = logsum over in-arcs (i -> j, pdf p, cost c) of alpha_t(i) - c + y_t(p);
//             log Z = logsum_i alpha_T(i) - final(i).
//   backward: beta_t(i) = logsum over out-arcs of -c + y_t(p) + beta_{t+1}(j); the arc's occupation
//             exp(alpha_t(i) - c + y_t(p) + beta_{t+1}(j) - log Z) goes to LDS, each pdf sums its arcs in a fixed
//             order, and the posterior is that sum over the sum of all the frame's occupations (1 up to rounding:
//             every path takes one arc per frame).
// A log-sum is two walks over the arc list, one for the maximum and one for the sum of exp(term - max) (fp32 exp of a
// difference, double log).  The probability domain with per-frame rescaling was tried first and dropped: over long
// utterances the forward share of a state that is on schedule for the final state decays exponentially while its
// backward value grows, so one of the two leaves the fp32 range (1200-frame utterances failed) whatever the rescaling.
// Threads own states (thread j walks the arc lists of states j, j + 256, ...) and distinct pdfs (thread k stages y and
// forms the posteriors of pdfs k, k + 256, ...); y of the next frame is loaded a frame ahead.  Three barriers per frame
// in each direction.  The alpha history and y of every (frame, pdf) live in the supervision's pool slot; y is overwritten
// by the backward pass with weight * posterior when the numerator runs beside the denominator ("staged").
// No float atomics, every sum in a fixed order: two runs give the same bits.
// A sequence beyond TC_E2E_MAX_STATES / _ARCS / _PDFS -- the occupations' LDS and the registers of a thread's pdfs -- takes
// num_e2e_large_kernels.hip, which keeps this kernel's arithmetic and orders (launch_num_e2e dispatches).
//
// The numerator's ok flag ([K] ComputeChainObjfAndDerivE2e: numerator_ok joins the denominator's and the finite check)
// rides on the sequence's log-probability: -inf when no path has T arcs, NaN when the backward total beta_0(start)
// disagrees with the forward one by more than kAgreeRel * max(1, |log Z|).  Either makes the objective non-finite, and
// finalize_kernel's check takes the soft-failure route for the whole minibatch.
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kE2ePdfsPerThread = TC_E2E_MAX_PDFS / kE2eThreads;

// the 256 threads' shares of a sequence's cross-entropy objective, added in a fixed order
__device__ __forceinline__ void e2e_xent_sum(double v, double *out, int tid) {
  __shared__ double xo_sh[kE2eThreads];
  __syncthreads();
  xo_sh[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < kE2eThreads; ++i) t += xo_sh[i];
    *out = t;
  }
}

}  // namespace

// RAGGED (a ragged supervision, NumParams::seq_frames): the sequence walks its own T_s frames; p.T stays the T of the tensors
// and of the scratch's strides (load_y, write_posterior, seq_view), so nothing at frames >= T_s is read or written.
template <typename El = float, bool RAGGED = false>
__global__ __launch_bounds__(kE2eThreads) void num_e2e_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int MS = (p.t.e2e_tab.max_states + 3) & ~3, MP = (p.t.e2e_tab.max_pdfs + 3) & ~3;
  double *A = reinterpret_cast<double *>(lds_raw);  // [2][MS]: log alpha (forward), log beta (backward), double-buffered
  float *E = reinterpret_cast<float *>(A + 2 * MS);  // [MP]: the frame's y per distinct pdf
  float *OCC = E + MP;                               // [max_arcs]: the frame's arc occupations (backward)
  __shared__ double red_d[4];
  __shared__ float red_c[4];

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? p.seq_frames[q] : p.T;
  const SeqView v = seq_view(p, q);
  const int start = p.t.e2e_tab.start[q];
  const bool want_beta = p.deriv != nullptr || p.xent != nullptr || p.seq_xent != nullptr;

  int pk[kE2ePdfsPerThread];  // the pdfs this thread owns (-1: none)
#pragma unroll
  for (int r = 0; r < kE2ePdfsPerThread; ++r) {
    const int k = tid + r * kE2eThreads;
    pk[r] = k < v.np ? v.pdf_of[k] : -1;
  }
  float ynx[kE2ePdfsPerThread];
#pragma unroll
  for (int r = 0; r < kE2ePdfsPerThread; ++r) ynx[r] = pk[r] >= 0 ? load_y<El>(p, q, 0, pk[r]) : 0.f;
  for (int i = tid; i < v.n; i += kE2eThreads) A[i] = i == start ? 0.0 : -INFINITY;

  // ---- forward ----
  int c = 0;
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int r = 0; r < kE2ePdfsPerThread; ++r) {
      if (pk[r] < 0) continue;
      const int k = tid + r * kE2eThreads;
      E[k] = ynx[r];
      if (want_beta) v.stage[(int64_t)t * v.np + k] = ynx[r];
      if (t + 1 < T) ynx[r] = load_y<El>(p, q, t + 1, pk[r]);  // a frame ahead
    }
    __syncthreads();
    const double *a_cur = A + c * MS;
    double *a_nxt = A + (1 - c) * MS;
    for (int j = tid; j < v.n; j += kE2eThreads) {
      if (want_beta) v.hist[(int64_t)t * v.n + j] = a_cur[j];
      double mx = -INFINITY;
      for (int i = v.in_begin[j]; i < v.in_begin[j + 1]; ++i) {
        const uint32_t key = v.in_key[i];
        mx = fmax(mx, a_cur[key & 0xffffu] + (double)(v.in_lw[i] + E[key >> 16]));
      }
      double acc = mx;
      if (mx > -INFINITY) {
        float sum = 0.f;
        for (int i = v.in_begin[j]; i < v.in_begin[j + 1]; ++i) {
          const uint32_t key = v.in_key[i];
          sum += __expf((float)(a_cur[key & 0xffffu] + (double)(v.in_lw[i] + E[key >> 16]) - mx));
        }
        acc = mx + log((double)sum);
      }
      a_nxt[j] = acc;
    }
    __syncthreads();
    c = 1 - c;
  }
  // log Z: logsum over the final states, by a fixed-order reduction
  double logz;
  {
    double mx = -INFINITY;
    for (int i = tid; i < v.n; i += kE2eThreads) {
      if (want_beta) v.hist[(int64_t)T * v.n + i] = A[c * MS + i];
      mx = fmax(mx, A[c * MS + i] + (double)v.final_lw[i]);
    }
    mx = e2e_wave_max_d(mx);
    if (lane == 0) red_d[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red_d[0], red_d[1]), fmax(red_d[2], red_d[3]));
    float sum = 0.f;
    if (mx > -INFINITY)
      for (int i = tid; i < v.n; i += kE2eThreads) sum += __expf((float)(A[c * MS + i] + (double)v.final_lw[i] - mx));
    sum = e2e_wave_sum(sum);
    if (lane == 0) red_c[wave] = sum;
    __syncthreads();
    logz = mx > -INFINITY ? mx + log((double)((red_c[0] + red_c[1]) + (red_c[2] + red_c[3]))) : -INFINITY;
  }
  if (!want_beta) {
    if (tid == 0) p.seq_logprob[q] = logz;
    return;
  }

  // ---- backward, with the posteriors ----
  const bool finite = logz - logz == 0.0;
  c = 0;
  for (int i = tid; i < v.n; i += kE2eThreads) A[i] = (double)v.final_lw[i];  // beta_T
  float enx[kE2ePdfsPerThread];
#pragma unroll
  for (int r = 0; r < kE2ePdfsPerThread; ++r)
    enx[r] = pk[r] >= 0 ? v.stage[(int64_t)(T - 1) * v.np + tid + r * kE2eThreads] : 0.f;
  double xo = 0.0;
  for (int t = T - 1; t >= 0; --t) {
#pragma unroll
    for (int r = 0; r < kE2ePdfsPerThread; ++r) {
      if (pk[r] < 0) continue;
      const int k = tid + r * kE2eThreads;
      E[k] = enx[r];
      if (t > 0) enx[r] = v.stage[(int64_t)(t - 1) * v.np + k];  // a frame ahead
    }
    __syncthreads();
    const double *b_cur = A + c * MS;
    double *b_nxt = A + (1 - c) * MS;
    for (int i = tid; i < v.n; i += kE2eThreads) {
      const double al = v.hist[(int64_t)t * v.n + i] - logz;
      double mx = -INFINITY;
      for (int a = v.out_begin[i]; a < v.out_begin[i + 1]; ++a) {
        const uint32_t key = v.out_key[a];
        const double x = (double)(v.out_lw[a] + E[key >> 16]) + b_cur[key & 0xffffu];
        mx = fmax(mx, x);
        OCC[a] = finite ? __expf((float)(al + x)) : 0.f;  // (exp(-inf) = 0: unreachable arcs)
      }
      double acc = mx;
      if (mx > -INFINITY) {
        float sum = 0.f;
        for (int a = v.out_begin[i]; a < v.out_begin[i + 1]; ++a) {
          const uint32_t key = v.out_key[a];
          sum += __expf((float)((double)(v.out_lw[a] + E[key >> 16]) + b_cur[key & 0xffffu] - mx));
        }
        acc = mx + log((double)sum);
      }
      b_nxt[i] = acc;
    }
    __syncthreads();
    float g[kE2ePdfsPerThread];
    float gs = 0.f;
#pragma unroll
    for (int r = 0; r < kE2ePdfsPerThread; ++r) {
      g[r] = 0.f;
      if (pk[r] < 0) continue;
      const int k = tid + r * kE2eThreads;
      for (int i = v.pdf_begin[k]; i < v.pdf_begin[k + 1]; ++i) g[r] += OCC[v.pdf_arc[i]];
      gs += g[r];
    }
    gs = e2e_wave_sum(gs);
    if (lane == 0) red_c[wave] = gs;
    __syncthreads();
    const float tot = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    const bool use = finite && tot > 0.f;  // (not the sign of rtot: a supervision weight may be negative)
    const float rtot = use ? p.weight / tot : 0.f;
#pragma unroll
    for (int r = 0; r < kE2ePdfsPerThread; ++r) {
      if (pk[r] < 0) continue;
      const int k = tid + r * kE2eThreads;
      const float val = use ? g[r] * rtot : 0.f;  // (no NaN from an infeasible sequence)
      if (p.staged)
        v.stage[(int64_t)t * v.np + k] = val;  // launch_num_e2e_scatter adds it once the denominator has written deriv
      else
        xo += write_posterior<El>(p, q, t, pk[r], val);
    }
    c = 1 - c;
  }
  if (tid == 0) {
    // beta_0(start) is log Z computed backward
    const double lb = A[c * MS + start];
    double out = logz;
    if (finite && !(fabs(lb - logz) <= (double)kAgreeRel * fmax(1.0, fabs(logz)))) out = NAN;
    p.seq_logprob[q] = out;
  }
  if (p.seq_xent && !p.staged) e2e_xent_sum(xo, p.seq_xent + q, tid);
}

// Second half of a staged e2e numerator: deriv[row, pdf] += weight * posterior, xent_deriv[row, pdf] = it.  Each
// (frame, pdf) of a sequence has one owner; the sequence's cross-entropy sum is added in a fixed order.
template <typename El = float, bool RAGGED = false>
__global__ __launch_bounds__(kE2eThreads) void num_e2e_scatter_kernel(const NumParams p) {
  const int q = blockIdx.x, tid = threadIdx.x;
  const E2eDev &e = p.t.e2e_tab;
  const int ub = e.pdf_off[q], np = e.pdf_off[q + 1] - ub;
  const float *stage = p.t.stage + (int64_t)p.T * ub;
  const int32_t *pdf_of = e.pdf_of + ub;
  double xo = 0.0;
  const int64_t n = (int64_t)(RAGGED ? p.seq_frames[q] : p.T) * np;  // (stage is [frame][upid]: the padding lies behind)
  for (int64_t i = tid; i < n; i += kE2eThreads) {
    const int t = (int)(i / np), k = (int)(i - (int64_t)t * np);
    xo += write_posterior<El>(p, q, t, pdf_of[k], stage[i]);
  }
  if (p.seq_xent) e2e_xent_sum(xo, p.seq_xent + q, tid);
}

int launch_num_e2e(const NumParams &p, hipStream_t stream) {
  const E2eDev &e = p.t.e2e_tab;
  // a sequence the resident kernel cannot hold, or the switch that sends the others there too: num_e2e_large_kernels.hip
  const bool large = e2e_beyond_resident(e.max_states, e.max_arcs, e.max_pdfs) || debug_flag(kDbgForceNumE2eLarge);
  // (... which needs the occupations' room in the slot: a handle staged before the switch was set has none.  Refused before
  // anything is counted)
  if (large && !e.occ_off256) return TC_ERR_UNSUPPORTED;
  count_launch(kCntNum);
  if (p.deriv || p.xent || p.seq_xent) count_launch(kCntNumBackward);
  if (p.staged) count_launch(kCntNumE2eStaged);  // (beside the denominator, posteriors left for the scatter kernel)
  if (large) return launch_num_e2e_large(p, stream);
  const size_t lds = num_e2e_lds_bytes(e.max_states, e.max_arcs, e.max_pdfs);
  void (*kernel)(const NumParams) = nullptr;
  if (p.seq_frames)
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_kernel<__hip_bfloat16, true>
             : p.elem == TC_DTYPE_F16 ? num_e2e_kernel<__half, true>
                                      : num_e2e_kernel<float, true>;
  else
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_kernel<__hip_bfloat16>
             : p.elem == TC_DTYPE_F16 ? num_e2e_kernel<__half>
                                      : num_e2e_kernel<float>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kE2eThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// (both forward-backward kernels leave their staged posteriors to this one: nothing in it depends on a sequence's size)
int launch_num_e2e_scatter(const NumParams &p, hipStream_t stream) {
  if (!p.deriv && !p.xent && !p.seq_xent) return TC_OK;
  void (*kernel)(const NumParams) = nullptr;
  if (p.seq_frames)
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_scatter_kernel<__hip_bfloat16, true>
             : p.elem == TC_DTYPE_F16 ? num_e2e_scatter_kernel<__half, true>
                                      : num_e2e_scatter_kernel<float, true>;
  else
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_scatter_kernel<__hip_bfloat16>
             : p.elem == TC_DTYPE_F16 ? num_e2e_scatter_kernel<__half>
                                      : num_e2e_scatter_kernel<float>;
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kE2eThreads), 0, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
