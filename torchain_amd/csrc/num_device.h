// The arithmetic of the regular numerator, shared by its two kernels: the resident one (num_kernels.hip: a whole
// sequence in LDS) and the level-windowed one (num_windowed_kernels.hip: two adjacent levels in LDS).  Both kernels form
// every value through these functions, operation for operation and in the same order, so that on a supervision both can
// run they give the same bits; they differ only in where an index finds its operand (the accessors they pass in).
#pragma once
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

__device__ __forceinline__ double log_add(double x, double y) {
  // [K] LogAdd(double, double), kMinLogDiffDouble = log(DBL_EPSILON)
  double diff;
  if (x < y) {
    diff = x - y;
    x = y;
  } else {
    diff = y - x;
  }
  if (diff >= -36.04365338911715) return x + log1p(exp(diff));
  return x;
}

// y at a sequence's unique (frame, pdf) entry `gu` (an index into uniq_t / uniq_pdf): [K] nnet_output_.Lookup(
// nnet_output_indexes_, ...); row = t*S + q.  E: element type of y when it is the caller's (B, C, T) tensor
template <typename E>
__device__ __forceinline__ float num_load_y(const NumParams &p, int q, int gu) {
  if constexpr (std::is_same<E, float>::value)
    return p.y_bct ? p.y[((int64_t)q * p.P + p.t.uniq_pdf[gu]) * p.T + p.t.uniq_t[gu]]
                   : p.y[((int64_t)p.t.uniq_t[gu] * p.S + q) * p.y_stride + p.t.uniq_pdf[gu]];
  else
    return p.y_bct ? load_elem<E>(p.y, ((int64_t)q * p.P + p.t.uniq_pdf[gu]) * p.T + p.t.uniq_t[gu])
                   : p.y[((int64_t)p.t.uniq_t[gu] * p.S + q) * p.y_stride + p.t.uniq_pdf[gu]];
}

// One state of either recursion: the log-sum, in list order, over the arcs arc_at(i0 .. i1) of score(a) (a float sum, as
// Kaldi) plus other(a), the log-alpha of the arc's source (forward, in-arc list) or the log-beta of its destination
// (backward, out-arcs; interior states are not final).
template <class ArcAt, class Score, class Other>
__device__ __forceinline__ double num_state_log_sum(int i0, int i1, ArcAt arc_at, Score score, Other other) {
  double acc = -INFINITY;
  for (int i = i0; i < i1; ++i) {
    const int a = arc_at(i);
    const float sc = score(a);
    acc = log_add(acc, (double)sc + other(a));
  }
  return acc;
}

// total: log-add over the final states st0 .. st1 in state order (one lane; a handful of states)
template <class Alpha>
__device__ __forceinline__ double num_total(int st0, int st1, const float *final_logw, Alpha alpha) {
  double tot = -INFINITY;
  for (int st = st0; st < st1; ++st)
    if (final_logw[st] != -INFINITY) tot = log_add(tot, alpha(st) + (double)final_logw[st]);
  return tot;
}

// occupation of an arc: exp(alpha(src) + score + beta(dst) - tot)
__device__ __forceinline__ float num_occupation(double alpha_src, float sc, double beta_dst, double tot) {
  const float occupation_logprob = (float)(alpha_src + (double)sc + beta_dst - tot);
  return __expf(occupation_logprob);
}

// weight * the posterior of one unique (frame, pdf): its arcs' occupations summed in uniq_arc order (the order Kaldi adds
// them)
template <class Occ>
__device__ __forceinline__ float num_posterior(const NumParams &p, const int *uniq_arc, int i0, int i1, Occ occ) {
  float sum = 0.f;
  for (int i = i0; i < i1; ++i) sum += occ(uniq_arc[i]);
  return p.weight * sum;
}

// The cross-entropy output element x of frame-major row `row` as the objective takes it: x itself, or with the row
// statistics of tc_chain_step_log_softmax (NumParams::xent_lse) the row's log-softmax x - max - log(sum(exp(x - max))), the
// two float32 statistics subtracted in double one after the other (a row shifted by 1e4 keeps its digits).
__device__ __forceinline__ double xent_log_prob(const NumParams &p, int64_t row, double x) {
  return p.xent_lse ? (x - (double)p.xent_lse[2 * row]) - (double)p.xent_lse[2 * row + 1] : x;
}

// scatter of one unique entry `gu` of sequence q: [K] AddElements(weight, indexes, derivs); v = weight * posterior.  Each
// (row, pdf) is owned by exactly one lane, so a plain read-modify-write.  Adds the entry's term of the sequence's
// cross-entropy objective to xo.
template <typename E>
__device__ __forceinline__ void num_scatter_one(const NumParams &p, int q, int gu, float v, double &xo) {
  const int64_t row = (int64_t)p.t.uniq_t[gu] * p.S + q;
  const int pdf = p.t.uniq_pdf[gu];
  // (scales other than 1 only through tc_chain_objf_and_grad: the reference's backward, -deriv and
  // -xent_regularize * xent_deriv, formed here instead of in two more passes over the matrices)
  if (p.deriv) p.deriv[row * p.deriv_stride + pdf] += p.deriv_scale * v;
  const int64_t bct = ((int64_t)q * p.P + pdf) * p.T + p.t.uniq_t[gu];  // (sequence, pdf, frame) of a (B, C, T) tensor
  if (p.xent) {  // (times the row's deriv_weight when one is given; the objective term below is not)
    const float xv = p.xent_scale * v;
    p.xent[p.xent_bct ? bct : row * p.xent_stride + pdf] = p.xent_row_w ? p.xent_row_w[row] * xv : xv;
  }
  // (the cross-entropy output: the caller's (B, C, T) tensor of element type E, or a float32 matrix)
  if (p.seq_xent)
    xo += (double)(p.xent_scale * v) * xent_log_prob(p, row, (double)(std::is_same<E, float>::value
                                                    ? p.xent_out[p.xent_out_bct ? bct : row * p.xent_out_stride + pdf]
                                                : p.xent_out_bct ? load_elem<E>(p.xent_out, bct)
                                                                 : p.xent_out[row * p.xent_out_stride + pdf]));
}

// The entries of a sequence are dealt to kNumScatterLanes lanes (entry u to lane u mod 128) whatever the workgroup's size,
// and the lanes' shares of the sequence's cross-entropy objective are added in lane order: the sum's order is one.
constexpr int kNumScatterLanes = 128;
__device__ __forceinline__ void seq_xent_sum(double v, double *out, int tid) {
  __shared__ double xo_sh[kNumScatterLanes];
  if (tid < kNumScatterLanes) xo_sh[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < kNumScatterLanes; ++i) t += xo_sh[i];
    *out = t;
  }
}

}  // namespace tc
