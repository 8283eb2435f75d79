// What the kernels that walk an end-to-end supervision share: a sequence's view of the tables (E2eDev) and the load of
// one network output.  num_e2e_kernels.hip (the forward-backward) and num_best_path_kernels.hip (the best path) both
// address the tables, the log-alpha history and y through these, so that both see the same operands.
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

}  // namespace tc
