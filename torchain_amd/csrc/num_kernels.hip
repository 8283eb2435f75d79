// Numerator forward-backward and the scalar epilogue of the chain objective for gfx950.
//
// [K] NumeratorComputation (chain-numerator.cc) runs a serial CPU loop over the merged supervision
// FST, bracketed by a device gather and a device scatter-add.  The merged FST factors per sequence
// (supervision.cpp), so here one workgroup of two wavefronts owns one sequence and walks its T time
// levels in LDS (one wave forward, one backward), in the log semiring and in double precision like Kaldi;
// lanes run over the states of a level.
// Occupation probabilities are summed per unique (frame, pdf) in arc order (the order Kaldi adds
// them), then added to the derivative with one plain read-modify-write per unique index -- each
// (row, pdf) is owned by exactly one lane, so no atomics.
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"

namespace tc {

// Two wavefronts per sequence: the alpha and the beta recursions do not depend on each other, so wave 0
// walks the levels forward while wave 1 walks them backward (T steps each, one shared barrier per step);
// the occupations need both and are computed afterwards, one arc per lane.  Per state the operations and
// their order are Kaldi's.
//
// STAGE: the sequence's own tables (level bounds, in / out offsets, in-arc list, arc source / destination / unique id /
// weight: a few KB) are copied into LDS first.  The T steps are one chain of dependent loads per step -- offsets ->
// arc ids -> arc fields -> alpha -- and from global memory every link was an L2 round trip: 0.73 us per step, 0.11 ms
// for 150 frames whatever the batch; from LDS the chain is a fraction of that.
// (the arithmetic itself is in num_device.h, shared with the level-windowed kernel)
// E: element type of y / xent_out when they are the caller's (B, C, T) tensors (NumParams::elem; 2-D: float32)
// RAGGED (a ragged supervision, NumParams::seq_frames): the sequence walks its own T_s frames, its level bounds start at
// seq_level_off[q]; p.T stays the T of the tensors (num_load_y, num_scatter_one) and of the LDS layout.  No padding row of
// y, deriv, xent or xent_out is touched: the tables hold the sequence's own frames only.
template <bool STAGE, typename E = float, bool RAGGED = false>
__global__ __launch_bounds__(128) void num_fwd_bwd_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *log_alpha = reinterpret_cast<double *>(lds_raw);
  double *log_beta = log_alpha + p.lds_states;
  float *ylp = reinterpret_cast<float *>(log_beta + p.lds_states);  // per unique (frame, pdf): y
  float *occ = ylp + p.lds_uniq;                                    // per arc: occupation prob
  int *s_in_begin = reinterpret_cast<int *>(occ + p.lds_arcs);      // STAGE: copies of the tables, in this order
  int *s_out_begin = s_in_begin + p.lds_states + 2;
  int *s_in_arc = s_out_begin + p.lds_states + 2;
  int *s_src = s_in_arc + p.lds_arcs;
  int *s_dst = s_src + p.lds_arcs;
  int *s_uq = s_dst + p.lds_arcs;
  float *s_lw = reinterpret_cast<float *>(s_uq + p.lds_arcs);
  int *s_level = reinterpret_cast<int *>(s_lw + p.lds_arcs);
  __shared__ double tot_sh;

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (a scalar: the frame loops and their barriers are the workgroup's)
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int sb = p.t.seq_state_off[q], nst = p.t.seq_state_off[q + 1] - sb;
  const int ab = p.t.seq_arc_off[q], narc = p.t.seq_arc_off[q + 1] - ab;
  const int ub = p.t.seq_uniq_off[q], nu = p.t.seq_uniq_off[q + 1] - ub;
  const int *g_level = p.t.level_begin + (RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(p.seq_level_off[q]) : (int64_t)q * (T + 2));
  const int *g_out_begin = p.t.out_begin + sb + q;
  const int *g_in_begin = p.t.in_begin + sb + q;
  const int *g_in_arc = p.t.in_arc + ab;
  const int *g_arc_src = p.t.arc_src + ab, *g_arc_dst = p.t.arc_dst + ab, *g_arc_uniq = p.t.arc_uniq + ab;
  const float *g_arc_logw = p.t.arc_logw + ab;
  if (STAGE) {
    for (int i = tid; i <= nst; i += 128) {
      s_in_begin[i] = g_in_begin[i];
      s_out_begin[i] = g_out_begin[i];
    }
    for (int a = tid; a < narc; a += 128) {
      s_in_arc[a] = g_in_arc[a];
      s_src[a] = g_arc_src[a];
      s_dst[a] = g_arc_dst[a];
      s_uq[a] = g_arc_uniq[a];
      s_lw[a] = g_arc_logw[a];
    }
    for (int i = tid; i < T + 2; i += 128) s_level[i] = g_level[i];
  }
  // (separate names per address space: a pointer that may be either would turn every access into a flat load)
  auto level = [&](int i) __attribute__((always_inline)) { return STAGE ? s_level[i] : g_level[i]; };
  auto in_begin = [&](int i) __attribute__((always_inline)) { return STAGE ? s_in_begin[i] : g_in_begin[i]; };
  auto out_begin = [&](int i) __attribute__((always_inline)) { return STAGE ? s_out_begin[i] : g_out_begin[i]; };
  auto in_arc = [&](int i) __attribute__((always_inline)) { return STAGE ? s_in_arc[i] : g_in_arc[i]; };
  auto arc_src = [&](int a) __attribute__((always_inline)) { return STAGE ? s_src[a] : g_arc_src[a]; };
  auto arc_dst = [&](int a) __attribute__((always_inline)) { return STAGE ? s_dst[a] : g_arc_dst[a]; };
  auto arc_uniq = [&](int a) __attribute__((always_inline)) { return STAGE ? s_uq[a] : g_arc_uniq[a]; };
  auto arc_logw = [&](int a) __attribute__((always_inline)) { return STAGE ? s_lw[a] : g_arc_logw[a]; };
  auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq(a)] + arc_logw(a); };
  const float *final_logw = p.t.final_logw + sb;
  const bool want_beta = p.deriv != nullptr || p.xent != nullptr || p.seq_xent != nullptr;

  // gather: [K] nnet_output_.Lookup(nnet_output_indexes_, ...); row = t*S + q
  for (int u = tid; u < nu; u += 128) ylp[u] = num_load_y<E>(p, q, ub + u);
  for (int i = tid; i < nst; i += 128) {
    log_alpha[i] = i == 0 ? 0.0 : -INFINITY;
    log_beta[i] = -INFINITY;
  }
  __syncthreads();
  if (wave == 1 && want_beta)
    for (int st = level(T) + lane; st < level(T + 1); st += 64) log_beta[st] = (double)final_logw[st];
  __syncthreads();

  for (int step = 0; step < T; ++step) {
    if (wave == 0) {
      // forward: level step+1 states take the log-sum over their in-arcs, in arc order
      const int l0 = level(step + 1), l1 = level(step + 2);
      for (int st = l0 + lane; st < l1; st += 64) {
        log_alpha[st] = num_state_log_sum(in_begin(st), in_begin(st + 1), in_arc, score,
                                          [&](int a) __attribute__((always_inline)) { return log_alpha[arc_src(a)]; });
      }
    } else if (want_beta) {
      // backward: level T-1-step states take the log-sum over their out-arcs
      const int t = T - 1 - step;
      const int l0 = level(t), l1 = level(t + 1);
      for (int st = l0 + lane; st < l1; st += 64) {
        log_beta[st] = num_state_log_sum(out_begin(st), out_begin(st + 1), [](int a) __attribute__((always_inline)) { return a; },
                                         score, [&](int a) __attribute__((always_inline)) { return log_beta[arc_dst(a)]; });
      }
    }
    __syncthreads();
  }
  // total: log-add over final states in state order (one lane; a handful of states)
  if (tid == 0) {
    const double tot = num_total(level(T), level(T + 1), final_logw,
                                 [&](int st) __attribute__((always_inline)) { return log_alpha[st]; });
    tot_sh = tot;
    p.seq_logprob[q] = tot;
  }
  __syncthreads();
  if (!want_beta) return;
  const double tot = tot_sh;
  // occupation of every arc: exp(alpha(src) + score + beta(dst) - tot)
  for (int a = tid; a < narc; a += 128) occ[a] = num_occupation(log_alpha[arc_src(a)], score(a), log_beta[arc_dst(a)], tot);
  __syncthreads();
  // scatter: [K] AddElements(weight, indexes, derivs)
  const int *uniq_begin = p.t.uniq_begin + ub + q;
  const int *uniq_arc = p.t.uniq_arc + ab;
  double xo = 0.0;
  for (int u = tid; u < nu; u += 128) {
    const float v = num_posterior(p, uniq_arc, uniq_begin[u], uniq_begin[u + 1],
                                  [&](int a) __attribute__((always_inline)) { return occ[a]; });
    if (p.staged) {
      p.t.stage[ub + u] = v;  // beside the denominator: launch_num_scatter adds it once deriv is written
      continue;
    }
    num_scatter_one<E>(p, q, ub + u, v, xo);
  }
  if (p.seq_xent && !p.staged) seq_xent_sum(xo, p.seq_xent + q, tid);
}

// Second half of a staged numerator: deriv[row, pdf] += weight * posterior, xent_deriv[row, pdf] = it, one owner
// per (row, pdf) as above.
template <typename E = float>
__global__ __launch_bounds__(128) void num_scatter_kernel(const NumParams p) {
  const int q = blockIdx.x;
  const int ub = p.t.seq_uniq_off[q], nu = p.t.seq_uniq_off[q + 1] - ub;
  double xo = 0.0;
  for (int u = threadIdx.x; u < nu; u += 128) {
    num_scatter_one<E>(p, q, ub + u, p.t.stage[ub + u], xo);
  }
  if (p.seq_xent) seq_xent_sum(xo, p.seq_xent + q, threadIdx.x);
}

int launch_num_scatter(const NumParams &p, hipStream_t stream) {
  if (p.t.e2e) return launch_num_e2e_scatter(p, stream);  // end-to-end supervision: num_e2e_kernels.hip
  if (!p.deriv && !p.xent && !p.seq_xent) return TC_OK;
  if (p.elem == TC_DTYPE_BF16)
    hipLaunchKernelGGL(num_scatter_kernel<__hip_bfloat16>, dim3(p.S), dim3(128), 0, stream, p);
  else if (p.elem == TC_DTYPE_F16)
    hipLaunchKernelGGL(num_scatter_kernel<__half>, dim3(p.S), dim3(128), 0, stream, p);
  else
    hipLaunchKernelGGL(num_scatter_kernel<float>, dim3(p.S), dim3(128), 0, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

namespace {
template <bool STAGE, typename E, bool RAGGED>
int launch_num_fwd_bwd(const NumParams &p, size_t lds, hipStream_t stream) {
  TC_HIP_CHECK(allow_dynamic_lds((const void *)num_fwd_bwd_kernel<STAGE, E, RAGGED>, lds));
  hipLaunchKernelGGL((num_fwd_bwd_kernel<STAGE, E, RAGGED>), dim3(p.S), dim3(128), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <bool STAGE, typename E>
int launch_num_fwd_bwd(const NumParams &p, size_t lds, hipStream_t stream) {
  if (p.seq_frames) {  // a ragged supervision: its own level offsets come with its lengths
    if (!p.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
    return launch_num_fwd_bwd<STAGE, E, true>(p, lds, stream);
  }
  return launch_num_fwd_bwd<STAGE, E, false>(p, lds, stream);
}

template <bool STAGE>
int launch_num_fwd_bwd(const NumParams &p, size_t lds, hipStream_t stream) {
  if (p.elem == TC_DTYPE_BF16) return launch_num_fwd_bwd<STAGE, __hip_bfloat16>(p, lds, stream);
  if (p.elem == TC_DTYPE_F16) return launch_num_fwd_bwd<STAGE, __half>(p, lds, stream);
  return launch_num_fwd_bwd<STAGE, float>(p, lds, stream);
}
}  // namespace

int launch_num(const NumParams &p, hipStream_t stream) {
  if (p.t.e2e) return launch_num_e2e(p, stream);  // end-to-end supervision: num_e2e_kernels.hip
  count_launch(kCntNum);
  if (p.deriv || p.xent || p.seq_xent) count_launch(kCntNumBackward);
  const size_t lds = (size_t)p.lds_states * 16 + (size_t)p.lds_uniq * 4 + (size_t)p.lds_arcs * 4;
  // a sequence that does not fit one workgroup's LDS: a window of levels instead (num_windowed_kernels.hip)
  if (lds > (size_t)kLdsLimitBytes || debug_flag(kDbgForceNumWindowed)) return launch_num_windowed(p, stream);
  // with the sequence's tables staged in LDS when that keeps a workgroup within a quarter of a CU's LDS (a ragged batch:
  // p.T is its longest sequence, as the maxima in p.lds_* are the batch's)
  const size_t staged = lds + ((size_t)2 * (p.lds_states + 2) + (size_t)5 * p.lds_arcs + (size_t)(p.T + 2)) * 4;
  if (staged <= (size_t)kLdsLimitBytes / 4) return launch_num_fwd_bwd<true>(p, staged, stream);
  return launch_num_fwd_bwd<false>(p, lds, stream);
}

// ---- scalar epilogue: [K] ComputeChainObjfAndDeriv after the two computations --------------------
__global__ __launch_bounds__(256) void finalize_kernel(const double *den_lp, const double *num_lp, const double *y2,
                                                       const float *ab, const float *gs, int S, int T,
                                                       float sup_weight, float l2, int have_deriv, float *results,
                                                       int32_t *fail_flag, const double *xent_lp, double *xent_total,
                                                       float *loss_out, int64_t total_frames) {
  __shared__ double sh[4][256];
  const int tid = threadIdx.x;
  double d = 0, n = 0, q = 0, a = 0, g = 0, x = 0;
  // fixed-order partial sums: thread i takes sequences i, i+256, ... (deterministic)
  for (int s = tid; s < S; s += 256) {
    d += den_lp[s];
    n += num_lp ? num_lp[s] : 0.0;
    q += y2[s];
    if (have_deriv) {
      a += (double)ab[s];
      g += (double)gs[s];
    }
    if (xent_lp) x += xent_lp[s];
  }
  sh[0][tid] = d;
  sh[1][tid] = n;
  sh[2][tid] = q;
  sh[3][tid] = a;
  __syncthreads();
  __shared__ double sh_g[256], sh_x[256];
  sh_g[tid] = g;
  sh_x[tid] = x;
  __syncthreads();
  if (tid == 0) {
    double D = 0, N = 0, Q = 0, A = 0, G = 0, X = 0;
    for (int i = 0; i < 256; ++i) {
      D += sh[0][i];
      N += sh[1][i];
      Q += sh[2][i];
      A += sh[3][i];
      G += sh_g[i];
      X += sh_x[i];
    }
    const float num_logprob_weighted = (float)(N * (double)sup_weight);
    const float den_logprob = (float)D;
    float objf = num_logprob_weighted - sup_weight * den_logprob;
    // (a ragged minibatch: its frames in all; y2 and the checks below already are per sequence over its own frames)
    const float weight = total_frames > 0 ? sup_weight * (float)total_frames : sup_weight * (float)S * (float)T;
    bool ok = true;
    if (have_deriv) {
      // [K] BetaGeneralFrameDebug(0)
      if (fabs(A - (double)S) > 2.0 || !(A - A == 0.0)) ok = false;
      if (fabs(G - (double)S) > 2.0 || !(G - G == 0.0)) ok = false;
    }
    int fail = 0;
    if (!(objf - objf == 0.0f) || !ok) {
      objf = -10.0f * weight;
      fail = 1;
    }
    float l2_term = 0.f;
    if (l2 != 0.0f) l2_term = (float)(-0.5 * (double)(sup_weight * l2) * (double)(float)Q);
    results[0] = objf;
    results[1] = l2_term;
    results[2] = weight;
    *fail_flag = fail;
    // tc_chain_step's two scalars ride along: the sequences' cross-entropy objective sums (NumParams::seq_xent; 0 after
    // a numerical failure, as the zeroed xent_deriv gives) and the loss -objf / weight (torchain/functions.py:104)
    if (xent_total) *xent_total = fail ? 0.0 : X;
    if (loss_out) loss_out[0] = -objf / weight;
  }
}

int launch_finalize(const double *den_lp, const double *num_lp, const double *y2, const float *ab, const float *gs,
                    int S, int T, float sup_weight, float l2, int have_deriv, float *results, int32_t *fail_flag,
                    hipStream_t stream, const double *xent_lp, double *xent_total, float *loss_out, int64_t total_frames) {
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, stream, den_lp, num_lp, y2, ab, gs, S, T, sup_weight, l2,
                     have_deriv, results, fail_flag, xent_lp, xent_total, loss_out, total_frames);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// ---- the scalar epilogue of tc_chain_step_per_sequence ------------------------------------------------------------
// finalize_kernel's sums twice, in its order (thread i takes sequences i, i + 256, ...; thread 0 adds the 256 partials):
// over every sequence, and over the sequences whose own scalars are all finite, a masked term being an exact +0.0.
// epilogue_scalars is finalize_kernel's arithmetic on one set of sums; `count` and `frames` are what the alpha-beta sums
// and the weight are held against (S and the minibatch's frames; the survivors' and theirs).
namespace {
struct EpilogueOut {
  float objf, l2_term, weight;
  int fail;
};

__device__ __forceinline__ EpilogueOut epilogue_scalars(double D, double N, double Q, double A, double G, double count,
                                                        float weight, float sup_weight, float l2, int have_deriv) {
  EpilogueOut e;
  const float num_logprob_weighted = (float)(N * (double)sup_weight);
  const float den_logprob = (float)D;
  float objf = num_logprob_weighted - sup_weight * den_logprob;
  bool ok = true;
  if (have_deriv) {
    if (fabs(A - count) > 2.0 || !(A - A == 0.0)) ok = false;
    if (fabs(G - count) > 2.0 || !(G - G == 0.0)) ok = false;
  }
  e.fail = 0;
  if (!(objf - objf == 0.0f) || !ok) {
    objf = -10.0f * weight;
    e.fail = 1;
  }
  e.l2_term = 0.f;
  if (l2 != 0.0f) e.l2_term = (float)(-0.5 * (double)(sup_weight * l2) * (double)(float)Q);
  e.objf = objf;
  e.weight = weight;
  return e;
}
}  // namespace

__global__ __launch_bounds__(256) void finalize_per_sequence_kernel(
    const double *den_lp, const double *num_lp, const double *y2, const float *ab, const float *gs, int S, int T,
    float sup_weight, float l2, int have_deriv, float *results, int32_t *fail_flag, const double *xent_lp, double *xent_total,
    float *loss_out, int64_t total_frames, const int32_t *seq_frames, int isolate, double *seq_results, int32_t *alive_frames) {
  __shared__ double sh[12][256];  // all: d n q a g x; alive: the same six
  __shared__ int sh_cnt[256];
  __shared__ long long sh_frames[256];
  __shared__ int sh_masked;
  const int tid = threadIdx.x;
  double d = 0, n = 0, q = 0, a = 0, g = 0, x = 0, md = 0, mn = 0, mq = 0, ma = 0, mg = 0, mx = 0;
  int cnt = 0;
  long long frames = 0;
  for (int s = tid; s < S; s += 256) {
    const double ds = den_lp[s], ns = num_lp ? num_lp[s] : 0.0, qs = y2[s];
    const double as = have_deriv ? (double)ab[s] : 0.0, gsv = have_deriv ? (double)gs[s] : 0.0;
    const double xs = xent_lp ? xent_lp[s] : 0.0;
    int own = T;
    if (seq_frames) {
      own = seq_frames[s];
      own = own < 1 ? 1 : (own > T ? T : own);
    }
    // (the sequence's cross-entropy sum is formed from the numerator's posteriors: non-finite with them)
    int status = 0;
    if (!(ns - ns == 0.0) || !(xs - xs == 0.0)) status |= 1;
    if (!(ds - ds == 0.0) || !(qs - qs == 0.0)) status |= 2;
    if (!(as - as == 0.0) || !(gsv - gsv == 0.0)) status |= 4;
    const bool alive = status == 0;
    d += ds;
    n += ns;
    q += qs;
    a += as;
    g += gsv;
    x += xs;
    md += alive ? ds : 0.0;
    mn += alive ? ns : 0.0;
    mq += alive ? qs : 0.0;
    ma += alive ? as : 0.0;
    mg += alive ? gsv : 0.0;
    mx += alive ? xs : 0.0;
    cnt += alive ? 1 : 0;
    frames += alive ? own : 0;
    if (seq_results) {
      double *r = seq_results + (int64_t)s * 6;
      r[0] = ns;
      r[1] = ds;
      r[2] = qs;
      r[3] = xs;
      r[4] = (double)own;
      r[5] = (double)status;
    }
    alive_frames[s] = alive ? own : 0;
  }
  sh[0][tid] = d;
  sh[1][tid] = n;
  sh[2][tid] = q;
  sh[3][tid] = a;
  sh[4][tid] = g;
  sh[5][tid] = x;
  sh[6][tid] = md;
  sh[7][tid] = mn;
  sh[8][tid] = mq;
  sh[9][tid] = ma;
  sh[10][tid] = mg;
  sh[11][tid] = mx;
  sh_cnt[tid] = cnt;
  sh_frames[tid] = frames;
  __syncthreads();
  if (tid == 0) {
    double t[12];
    for (int k = 0; k < 12; ++k) t[k] = 0;
    int alive_n = 0;
    long long alive_f = 0;
    for (int i = 0; i < 256; ++i) {
      for (int k = 0; k < 12; ++k) t[k] += sh[k][i];
      alive_n += sh_cnt[i];
      alive_f += sh_frames[i];
    }
    // finalize_kernel's weight and outputs, from the sums over every sequence
    const float weight_all = total_frames > 0 ? sup_weight * (float)total_frames : sup_weight * (float)S * (float)T;
    EpilogueOut e = epilogue_scalars(t[0], t[1], t[2], t[3], t[4], (double)S, weight_all, sup_weight, l2, have_deriv);
    double X = t[5];
    int masked = 0;
    if (isolate && alive_n > 0 && alive_n < S) {
      // the survivors: their sums, their count, their frames (the weight in the form of the minibatch's own)
      const float weight_m = total_frames > 0 ? sup_weight * (float)alive_f : sup_weight * (float)alive_n * (float)T;
      const EpilogueOut m = epilogue_scalars(t[6], t[7], t[8], t[9], t[10], (double)alive_n, weight_m, sup_weight, l2, have_deriv);
      if (!m.fail) {  // (else the whole minibatch takes the failure route, as without the switch)
        e = m;
        X = t[11];
        masked = 1;
      }
    }
    sh_masked = masked;
    results[0] = e.objf;
    results[1] = e.l2_term;
    results[2] = e.weight;
    *fail_flag = e.fail;
    if (xent_total) *xent_total = e.fail ? 0.0 : X;
    if (loss_out) loss_out[0] = -e.objf / e.weight;
  }
  __syncthreads();
  if (!sh_masked) {  // nothing is masked out: every sequence keeps its own frames
    for (int s = tid; s < S; s += 256) {
      int own = T;
      if (seq_frames) {
        own = seq_frames[s];
        own = own < 1 ? 1 : (own > T ? T : own);
      }
      alive_frames[s] = own;
    }
  }
}

int launch_finalize_per_sequence(const double *den_lp, const double *num_lp, const double *y2, const float *ab, const float *gs,
                                 int S, int T, float sup_weight, float l2, int have_deriv, float *results, int32_t *fail_flag,
                                 hipStream_t stream, const double *xent_lp, double *xent_total, float *loss_out,
                                 int64_t total_frames, const int32_t *seq_frames, int isolate, double *seq_results,
                                 int32_t *alive_frames) {
  if (!alive_frames) return TC_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(finalize_per_sequence_kernel, dim3(1), dim3(256), 0, stream, den_lp, num_lp, y2, ab, gs, S, T, sup_weight,
                     l2, have_deriv, results, fail_flag, xent_lp, xent_total, loss_out, total_frames, seq_frames, isolate,
                     seq_results, alive_frames);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// Resets the derivative outputs when the finalize step flagged a numerical failure (rare path; exits
// after one uniform load otherwise).  [K] zeroes both derivatives and only then adds the l2 term, so
// deriv becomes -l2_scale*y and xent_deriv 0.
__global__ __launch_bounds__(256) void zero_on_fail_kernel(const int32_t *fail_flag, float *a, int64_t a_stride,
                                                           float *b, int64_t b_stride, const float *y,
                                                           int64_t y_stride, float l2_scale, int64_t rows, int cols) {
  if (*fail_flag == 0) return;
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    if (a) a[r * a_stride + c] = -l2_scale * y[r * y_stride + c];
    if (b) b[r * b_stride + c] = 0.f;
  }
}

int launch_zero_on_fail(const int32_t *fail_flag, float *a, int64_t a_stride, float *b, int64_t b_stride,
                        const float *y, int64_t y_stride, float l2_scale, int64_t rows, int cols,
                        hipStream_t stream) {
  if (!a && !b) return TC_OK;
  hipLaunchKernelGGL(zero_on_fail_kernel, dim3(1024), dim3(256), 0, stream, fail_flag, a, a_stride, b, b_stride, y, y_stride,
                     l2_scale, rows, cols);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// Reduction used by the split entry point tc_den_forward_backward.
__global__ __launch_bounds__(256) void den_reduce_kernel(const double *den_lp, const float *ab, const float *gs, int S,
                                                         double *logprob_out, int32_t *status_out) {
  __shared__ double sh[3][256];
  const int tid = threadIdx.x;
  double d = 0, a = 0, g = 0;
  for (int s = tid; s < S; s += 256) {
    d += den_lp[s];
    if (ab) {
      a += (double)ab[s];
      g += (double)gs[s];
    }
  }
  sh[0][tid] = d;
  sh[1][tid] = a;
  sh[2][tid] = g;
  __syncthreads();
  if (tid == 0) {
    double D = 0, A = 0, G = 0;
    for (int i = 0; i < 256; ++i) {
      D += sh[0][i];
      A += sh[1][i];
      G += sh[2][i];
    }
    if (logprob_out) *logprob_out = D;
    if (status_out) {
      int bad = 0;
      if (!(D - D == 0.0)) bad = 1;
      if (ab && (fabs(A - (double)S) > 2.0 || fabs(G - (double)S) > 2.0 || !(A - A == 0.0) || !(G - G == 0.0))) bad = 1;
      *status_out = bad;
    }
  }
}

int launch_den_reduce(const double *den_lp, const float *ab, const float *gs, int S, double *logprob_out,
                      int32_t *status_out, hipStream_t stream) {
  hipLaunchKernelGGL(den_reduce_kernel, dim3(1), dim3(256), 0, stream, den_lp, ab, gs, S, logprob_out, status_out);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

__global__ __launch_bounds__(256) void sum_double_kernel(const double *in, int n, double scale, double *out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double d = 0;
  for (int i = tid; i < n; i += 256) d += in[i];
  sh[tid] = d;
  __syncthreads();
  if (tid == 0) {
    double D = 0;
    for (int i = 0; i < 256; ++i) D += sh[i];
    *out = D * scale;
  }
}

// tc_chain_step: loss = -objf / weight (the reference's input.new([results.loss]), torchain/functions.py:104) on the device
__global__ void step_loss_kernel(const float *results3, float *loss1) { loss1[0] = -results3[0] / results3[2]; }

int launch_step_loss(const float *results3, float *loss1, hipStream_t stream) {
  hipLaunchKernelGGL(step_loss_kernel, dim3(1), dim3(1), 0, stream, results3, loss1);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

// the sequences' cross-entropy objective sums (NumParams::seq_xent) -> their total; 0 after a numerical failure, as the
// zeroed xent_deriv gives
__global__ __launch_bounds__(256) void xent_total_kernel(const double *in, int n, const int32_t *fail_flag, double *out) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  double d = 0;
  for (int i = tid; i < n; i += 256) d += in[i];
  sh[tid] = d;
  __syncthreads();
  if (tid == 0) {
    double D = 0;
    for (int i = 0; i < 256; ++i) D += sh[i];
    *out = *fail_flag ? 0.0 : D;
  }
}

int launch_xent_total(const double *in, int n, const int32_t *fail_flag, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(xent_total_kernel, dim3(1), dim3(256), 0, stream, in, n, fail_flag, out);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

int launch_sum_double(const double *in, int n, double scale, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(sum_double_kernel, dim3(1), dim3(256), 0, stream, in, n, scale, out);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
