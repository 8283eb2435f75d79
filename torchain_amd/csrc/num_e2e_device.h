// What the kernels that walk an end-to-end supervision share: a sequence's view of the tables (E2eDev) and the load of
// one network output.  num_e2e_kernels.hip and num_e2e_large_kernels.hip (the forward-backward, for sequences that fit on
// chip and for those that do not) and num_best_path_kernels.hip (the best path) all address the tables, the log-alpha
// history and y through these, so that they see the same operands; the two forward-backward kernels also share the wave
// reductions and the write of a posterior, so that they give the same bits.
#pragma once

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

struct SeqView {
  int n, na, np, sb, ub;
  const int32_t *in_begin, *out_begin, *pdf_begin, *pdf_arc, *pdf_of;
  const uint32_t *in_key, *out_key;
  const float *in_lw, *out_lw, *final_lw;
  double *hist;
  float *stage;
};

__device__ __forceinline__ SeqView seq_view(const NumParams &p, int q) {
  const E2eDev &e = p.t.e2e_tab;
  SeqView v;
  v.sb = e.state_off[q];
  v.n = e.state_off[q + 1] - v.sb;
  const int ab = e.arc_off[q];
  v.na = e.arc_off[q + 1] - ab;
  v.ub = e.pdf_off[q];
  v.np = e.pdf_off[q + 1] - v.ub;
  v.in_begin = e.in_begin + v.sb + q;
  v.out_begin = e.out_begin + v.sb + q;
  v.pdf_begin = e.pdf_begin + v.ub + q;
  v.pdf_arc = e.pdf_arc + ab;
  v.pdf_of = e.pdf_of + v.ub;
  v.in_key = e.in_key + ab;
  v.out_key = e.out_key + ab;
  v.in_lw = e.in_lw + ab;
  v.out_lw = e.out_lw + ab;
  v.final_lw = e.final_lw + v.sb;
  v.hist = e.alpha_hist + (int64_t)(p.T + 1) * v.sb;
  v.stage = p.t.stage + (int64_t)p.T * v.ub;
  return v;
}

// El: element type of y / xent_out when they are the caller's (B, C, T) tensors (NumParams::elem; 2-D: float32)
template <typename El>
__device__ __forceinline__ float load_y(const NumParams &p, int q, int t, int pdf) {
  return p.y_bct ? load_elem<El>(p.y, ((int64_t)q * p.P + pdf) * p.T + t) : p.y[((int64_t)t * p.S + q) * p.y_stride + pdf];
}

// ---- what the two forward-backward kernels (num_e2e_kernels.hip, num_e2e_large_kernels.hip) share beyond that ----
constexpr int kE2eThreads = 256;
constexpr float kAgreeRel = 1e-4f;

__device__ __forceinline__ float e2e_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double e2e_wave_max_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// the sequence's posterior v = weight * gamma of (frame t, pdf) into deriv / xent, and its cross-entropy objective term
template <typename El>
__device__ __forceinline__ double write_posterior(const NumParams &p, int q, int t, int pdf, float v) {
  const int64_t row = (int64_t)t * p.S + q;
  const int64_t bct = ((int64_t)q * p.P + pdf) * p.T + t;  // (sequence, pdf, frame) of a (B, C, T) tensor
  if (p.deriv) p.deriv[row * p.deriv_stride + pdf] += p.deriv_scale * v;
  if (p.xent) {  // (times the row's deriv_weight when one is given; the objective term below is not)
    const float xv = p.xent_scale * v;
    p.xent[p.xent_bct ? bct : row * p.xent_stride + pdf] = p.xent_row_w ? p.xent_row_w[row] * xv : xv;
  }
  if (p.seq_xent) {
    const double x = (double)(std::is_same<El, float>::value
                                  ? p.xent_out[p.xent_out_bct ? bct : row * p.xent_out_stride + pdf]
                                  : p.xent_out_bct ? load_elem<El>(p.xent_out, bct)
                                                   : p.xent_out[row * p.xent_out_stride + pdf]);
    // (tc_chain_step_log_softmax: the row's log-softmax, as num_device.h's xent_log_prob states it)
    return (double)(p.xent_scale * v) * (p.xent_lse ? (x - (double)p.xent_lse[2 * row]) - (double)p.xent_lse[2 * row + 1] : x);
  }
  return 0.0;
}

}  // namespace tc
