// Numerator of end-to-end supervisions whose sequences do not fit num_e2e_kernel (num_e2e_kernels.hip), for gfx950.
//
// The resident kernel keeps a frame's arc occupations in LDS, one float per arc, and the distinct pdfs a thread owns in
// registers: TC_E2E_MAX_STATES / _ARCS / _PDFS.  An acceptor composed with the denominator graph's normalization acceptor,
// or a long transcript's, is past them.  This kernel is the same computation -- one workgroup of 256 threads per sequence,
// the same tables (SeqView), the same log-semiring arithmetic (double alpha and beta, fp32 exp of a difference, double
// log), the same orders of every sum, the same failure conventions -- with the two things that set those limits moved:
//   - the arc occupations go to the supervision's pool slot (E2eDev::occ_off256), 4 bytes per arc.  The thread that owns a
//     state stores its out-arcs' occupations; after the workgroup's barrier the thread that owns a pdf loads them in
//     pdf_arc's order.  __syncthreads() is a workgroup-scope release and acquire: every wave waits for its own vector
//     stores (vmcnt(0)) before the barrier, and the waves of a workgroup share their CU's vector L1, so the loads behind
//     the barrier see the stores in front of it (the best path's traceback reads the score history the same way);
//   - the distinct pdfs are walked k = tid, tid + 256, ...: y is staged without a frame of look-ahead, and a pdf's
//     occupation sum waits in its own E[k] (no state reads E after the frame's barrier) for the frame's total.
// What is left in LDS is two double score vectors and the frame's y per distinct pdf, 16 * states + 4 * pdfs bytes laid out
// with the sequence's own sizes (the create rule is per sequence), and 48 bytes of reduction cells: the cross-entropy
// shares are added wave by wave over shuffles, in the resident kernel's order, not through a 2 KiB array.  The arc count of
// a sequence is not limited.
//
// On a supervision that fits both, this kernel gives the resident kernel's bits (tc_debug_set("force_num_e2e_large", 1)):
// log-probabilities, derivative, xent derivative and xent objective.  The staged posteriors go through the resident file's
// scatter kernel, which depends on no size.  What it costs: profiles/e2e_large/README.md.
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

// the 256 threads' shares of a sequence's cross-entropy objective, added in thread order as e2e_xent_sum adds them:
// wave w continues the running total of wave w - 1, which waits in one LDS cell
__device__ __forceinline__ void e2e_xent_sum_waves(double v, double *out, double *cell, int lane, int wave) {
  for (int w = 0; w < kE2eThreads / 64; ++w) {
    __syncthreads();
    if (wave != w) continue;
    double t = w == 0 ? 0.0 : *cell;
    for (int i = 0; i < 64; ++i) t += __shfl(v, i, 64);
    if (lane == 0) *(w == kE2eThreads / 64 - 1 ? out : cell) = t;
  }
}

}  // namespace

// El, RAGGED: as num_e2e_kernel's.
template <typename El = float, bool RAGGED = false>
__global__ __launch_bounds__(kE2eThreads) void num_e2e_large_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_d[4];
  __shared__ float red_c[4];

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? p.seq_frames[q] : p.T;
  const SeqView v = seq_view(p, q);
  // the sequence's own layout: the create rule holds for every sequence, not for the batch's largest state count beside
  // its largest pdf count, which may belong to two sequences
  const int MS = (v.n + 3) & ~3;
  double *A = reinterpret_cast<double *>(lds_raw);   // [2][MS]: log alpha (forward), log beta (backward), double-buffered
  float *E = reinterpret_cast<float *>(A + 2 * MS);  // [v.np]: the frame's y per distinct pdf; then its occupation sum
  const int start = p.t.e2e_tab.start[q];
  const bool want_beta = p.deriv != nullptr || p.xent != nullptr || p.seq_xent != nullptr;
  // the sequence's arc occupations, in the slot (out-arc positions, as the resident kernel's OCC)
  float *occ = reinterpret_cast<float *>(reinterpret_cast<char *>(p.t.e2e_tab.alpha_hist) + (int64_t)p.t.e2e_tab.occ_off256 * 256) +
               p.t.e2e_tab.arc_off[q];

  for (int i = tid; i < v.n; i += kE2eThreads) A[i] = i == start ? 0.0 : -INFINITY;

  // ---- forward ----
  int c = 0;
  for (int t = 0; t < T; ++t) {
    for (int k = tid; k < v.np; k += kE2eThreads) {
      const float yv = load_y<El>(p, q, t, v.pdf_of[k]);
      E[k] = yv;
      if (want_beta) v.stage[(int64_t)t * v.np + k] = yv;
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
  // log Z: logsum over the final states, by the resident kernel's fixed-order reduction
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
  double xo = 0.0;
  for (int t = T - 1; t >= 0; --t) {
    for (int k = tid; k < v.np; k += kE2eThreads) E[k] = v.stage[(int64_t)t * v.np + k];
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
        occ[a] = finite ? __expf((float)(al + x)) : 0.f;  // (exp(-inf) = 0: unreachable arcs)
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
    __syncthreads();  // (the occupations' stores before their loads: see the head of the file)
    float gs = 0.f;
    for (int k = tid; k < v.np; k += kE2eThreads) {
      float g = 0.f;
      for (int i = v.pdf_begin[k]; i < v.pdf_begin[k + 1]; ++i) g += occ[v.pdf_arc[i]];
      E[k] = g;  // (this thread's own cell; y of the frame is done with)
      gs += g;
    }
    gs = e2e_wave_sum(gs);
    if (lane == 0) red_c[wave] = gs;
    __syncthreads();
    const float tot = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    const bool use = finite && tot > 0.f;  // (not the sign of rtot: a supervision weight may be negative)
    const float rtot = use ? p.weight / tot : 0.f;
    for (int k = tid; k < v.np; k += kE2eThreads) {
      const float val = use ? E[k] * rtot : 0.f;  // (no NaN from an infeasible sequence)
      if (p.staged)
        v.stage[(int64_t)t * v.np + k] = val;  // launch_num_e2e_scatter adds it once the denominator has written deriv
      else
        xo += write_posterior<El>(p, q, t, v.pdf_of[k], val);
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
  if (p.seq_xent && !p.staged) e2e_xent_sum_waves(xo, p.seq_xent + q, red_d, lane, wave);
}

int launch_num_e2e_large(const NumParams &p, hipStream_t stream) {
  const E2eDev &e = p.t.e2e_tab;
  // (a handle that fits the resident kernel and reached the device before "force_num_e2e_large" was set has no room for
  // the occupations in its slot: launch_num_e2e has refused it)
  if (!e.occ_off256) return TC_ERR_UNSUPPORTED;
  count_launch(kCntNumE2eLarge);
  const size_t lds = e2e_seq_lds_bytes(e.max_states, e.max_pdfs);
  void (*kernel)(const NumParams) = nullptr;
  if (p.seq_frames)
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_large_kernel<__hip_bfloat16, true>
             : p.elem == TC_DTYPE_F16 ? num_e2e_large_kernel<__half, true>
                                      : num_e2e_large_kernel<float, true>;
  else
    kernel = p.elem == TC_DTYPE_BF16 ? num_e2e_large_kernel<__hip_bfloat16>
             : p.elem == TC_DTYPE_F16 ? num_e2e_large_kernel<__half>
                                      : num_e2e_large_kernel<float>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kE2eThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
