// Level-windowed numerator forward-backward for gfx950: regular supervisions whose sequences do not fit the resident
// kernel's LDS (num_kernels.hip keeps every state, arc and unique (frame, pdf) of a sequence on chip).
//
// The supervision FST is unfolded in time (supervision.cpp): states are numbered level by level, the in-arcs of a level
// t+1 state all leave level t, the arcs leaving level t are one contiguous range of arc ids, and so are the unique
// (frame, pdf) entries of frame t.  The recursions therefore need two adjacent levels at a time.  One workgroup of four
// wavefronts owns one sequence and keeps in LDS, sized by the widest level of the batch:
//   log-alpha and log-beta of the current and the next level (double, ping-pong), y of the frame's unique entries,
//   the occupations of the frame's arcs.
// Forward: T steps; the log-alpha of every state also goes to the history in global memory (NumDev::alpha_hist, one
// double per state, in the supervision's pool slot; not written by a forward-only call).  Backward: T steps from the
// last frame; a step reads its level's log-alpha back, forms the level's log-beta and the occupations of the arcs that
// leave it -- both need only the next level's log-beta -- and then every unique entry of the frame sums its arcs and
// leaves weight * posterior in NumDev::stage.  Afterwards the entries are scattered exactly as num_scatter_kernel does
// it (entry u on lane u mod 128), here or, beside the denominator, by that kernel.
//
// Every value is formed by the functions of num_device.h that the resident kernel uses, on the same operands in the same
// order: on a supervision that fits both, the two kernels give the same bits.  The tables are read from global memory
// (L2): the levels that need this kernel are wide, so a step's loads are many independent chains over 256 lanes rather
// than the one dependent chain per step that made the resident kernel stage its tables.
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"

namespace tc {

constexpr int kWinThreads = 256;

// E: element type of y / xent_out when they are the caller's (B, C, T) tensors (NumParams::elem; 2-D: float32)
// RAGGED (a ragged supervision, NumParams::seq_frames): the sequence walks its own T_s frames; its level bounds start at
// seq_level_off[q] and its frame_uniq entries at seq_level_off[q] - q (one entry fewer per sequence); p.T stays the T of the
// tensors.  No padding row is touched.
template <typename E = float, bool RAGGED = false>
__global__ __launch_bounds__(kWinThreads) void num_windowed_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *alpha_w = reinterpret_cast<double *>(lds_raw);  // [2][win_states]
  double *beta_w = alpha_w + 2 * p.win_states;            // [2][win_states]
  float *ylp = reinterpret_cast<float *>(beta_w + 2 * p.win_states);  // per unique (frame, pdf) of the frame: y
  float *occ = ylp + p.win_uniq;                                      // per arc leaving the level: occupation prob
  __shared__ double tot_sh;

  const int q = blockIdx.x, tid = threadIdx.x;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T, W = p.win_states;  // (T: a scalar, as the barriers need)
  const int64_t lo = RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(p.seq_level_off[q]) : (int64_t)q * (T + 2);
  const int sb = p.t.seq_state_off[q];
  const int ab = p.t.seq_arc_off[q];
  const int ub = p.t.seq_uniq_off[q], nu = p.t.seq_uniq_off[q + 1] - ub;
  const int *level = p.t.level_begin + lo;
  const int *frame_uniq = p.t.frame_uniq + (RAGGED ? lo - q : (int64_t)q * (T + 1));
  const int *out_begin = p.t.out_begin + sb + q;
  const int *in_begin = p.t.in_begin + sb + q;
  const int *in_arc = p.t.in_arc + ab;
  const int *arc_src = p.t.arc_src + ab, *arc_dst = p.t.arc_dst + ab, *arc_uniq = p.t.arc_uniq + ab;
  const float *arc_logw = p.t.arc_logw + ab;
  const float *final_logw = p.t.final_logw + sb;
  double *hist = p.t.alpha_hist + sb;
  const bool want_beta = p.deriv != nullptr || p.xent != nullptr || p.seq_xent != nullptr;

  // ---- forward: level t -> level t + 1 ----
  if (tid == 0) {
    alpha_w[0] = 0.0;  // level 0 is the start state alone
    if (want_beta) hist[0] = 0.0;
  }
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    for (int u = u0 + tid; u < u1; u += kWinThreads) ylp[u - u0] = num_load_y<E>(p, q, ub + u);
    __syncthreads();
    const double *cur = alpha_w + (t & 1) * W;
    double *nxt = alpha_w + ((t + 1) & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s1 + tid; st < s2; st += kWinThreads) {
      const double v = num_state_log_sum(in_begin[st], in_begin[st + 1],
                                         [&](int i) __attribute__((always_inline)) { return in_arc[i]; }, score,
                                         [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
      nxt[st - s1] = v;
      if (want_beta) hist[st] = v;
    }
    __syncthreads();
  }
  const int f0 = level[T], f1 = level[T + 1];
  if (tid == 0) {
    const double *last = alpha_w + (T & 1) * W;
    const double tot = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
    tot_sh = tot;
    p.seq_logprob[q] = tot;
  }
  if (!want_beta) return;
  for (int st = f0 + tid; st < f1; st += kWinThreads) beta_w[(T & 1) * W + st - f0] = (double)final_logw[st];
  __syncthreads();
  const double tot = tot_sh;

  // ---- backward: level t + 1 -> level t, and the posteriors of frame t ----
  const int *uniq_begin = p.t.uniq_begin + ub + q;
  const int *uniq_arc = p.t.uniq_arc + ab;
  double *alpha_t = alpha_w;
  for (int t = T - 1; t >= 0; --t) {
    const int s0 = level[t], s1 = level[t + 1];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    for (int u = u0 + tid; u < u1; u += kWinThreads) ylp[u - u0] = num_load_y<E>(p, q, ub + u);
    for (int st = s0 + tid; st < s1; st += kWinThreads) alpha_t[st - s0] = hist[st];
    __syncthreads();
    const double *nxt = beta_w + ((t + 1) & 1) * W;
    double *cur = beta_w + (t & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s0 + tid; st < s1; st += kWinThreads)
      cur[st - s0] = num_state_log_sum(out_begin[st], out_begin[st + 1], [](int a) __attribute__((always_inline)) { return a; },
                                       score, [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1]; });
    for (int a = a0 + tid; a < a1; a += kWinThreads)
      occ[a - a0] = num_occupation(alpha_t[arc_src[a] - s0], score(a), nxt[arc_dst[a] - s1], tot);
    __syncthreads();
    for (int u = u0 + tid; u < u1; u += kWinThreads)
      p.t.stage[ub + u] = num_posterior(p, uniq_arc, uniq_begin[u], uniq_begin[u + 1],
                                        [&](int a) __attribute__((always_inline)) { return occ[a - a0]; });
    __syncthreads();
  }
  if (p.staged) return;  // beside the denominator: launch_num_scatter adds the posteriors once deriv is written
  // scatter, as num_scatter_kernel: entry u on lane u mod kNumScatterLanes (the stage writes above are this workgroup's
  // own, ordered before these reads by the barrier)
  double xo = 0.0;
  if (tid < kNumScatterLanes)
    for (int u = tid; u < nu; u += kNumScatterLanes) num_scatter_one<E>(p, q, ub + u, p.t.stage[ub + u], xo);
  if (p.seq_xent) seq_xent_sum(xo, p.seq_xent + q, tid);
}

namespace {
template <typename E, bool RAGGED>
int launch_windowed(const NumParams &p, size_t lds, hipStream_t stream) {
  TC_HIP_CHECK(allow_dynamic_lds((const void *)num_windowed_kernel<E, RAGGED>, lds));
  hipLaunchKernelGGL((num_windowed_kernel<E, RAGGED>), dim3(p.S), dim3(kWinThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_windowed(const NumParams &p, size_t lds, hipStream_t stream) {
  if (p.seq_frames) {  // a ragged supervision: its own level offsets come with its lengths
    if (!p.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
    return launch_windowed<E, true>(p, lds, stream);
  }
  return launch_windowed<E, false>(p, lds, stream);
}
}  // namespace

int launch_num_windowed(const NumParams &p, hipStream_t stream) {
  const size_t lds = (size_t)p.win_states * 32 + (size_t)p.win_uniq * 4 + (size_t)p.win_arcs * 4;
  if (!num_windowed_fits(lds) || !p.t.alpha_hist || !p.t.frame_uniq) return TC_ERR_UNSUPPORTED;
  count_launch(kCntNumWindowed);
  if (p.elem == TC_DTYPE_BF16) return launch_windowed<__hip_bfloat16>(p, lds, stream);
  if (p.elem == TC_DTYPE_F16) return launch_windowed<__half>(p, lds, stream);
  return launch_windowed<float>(p, lds, stream);
}

}  // namespace tc
