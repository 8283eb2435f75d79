// Wide-level numerator forward-backward for gfx950: regular supervisions with a time level too wide for the level-windowed
// kernel (num_windowed_kernels.hip keeps log-alpha and log-beta of two adjacent levels, y and the occupations of a frame in
// LDS: 32 bytes a state and 4 an arc of the widest level).  Here no per-level vector has to fit LDS, so no level is
// refused on size.  Taken only by a handle that allows it (tc_supervision_allow_wide_levels), after the resident and the
// windowed kernel (launch_num).
//
// The supervision is unfolded in time as the windowed kernel's header says: the in-arcs of a level t+1 state leave level t,
// the arcs leaving a level are one range of arc ids sorted by source, the unique (frame, pdf) entries of a frame are one
// range.  A level has thousands of independent states and arcs, so ONE WORKGROUP OF 1024 THREADS (16 waves) owns a sequence
// and walks its levels; a step's loads are sixteen waves of independent chains.
//
// What a step addresses at random is one per-state vector, the GATHER VECTOR: log-alpha of level t, gathered through
// arc_src by the states of level t+1 (forward); log-beta of level t+1, gathered through arc_dst by the states and arcs of
// level t (backward).  It and y of the frame's unique entries are all that LDS holds (8 bytes a state, 4 an entry).
// Everything else streams through the supervision's pool slot with unit-stride accesses:
//   log-alpha of every state -> the history NumDev::alpha_hist (written by forward-only calls too: it is the next step's
//                               gather source); the backward pass reads log-alpha of an arc's source from it where it lies
//                               (arcs are sorted by source: nearly unit stride);
//   log-beta                 -> two level-sized rows, ping-pong (NumParams::wide_rows);
//   occupations of the arcs leaving the level -> one level-sized float row behind them.
// After the barrier that ends a step, the row it wrote is loaded into LDS as the next step's gather vector.  Two barriers a
// level in either direction.
//
// SLOT form (a level beyond the LDS form's rule 8 * ceil2(states) + 4 * ceil4(frame's entries) + 2048 <= 163840, about 20000
// states; or "force_num_wide_streamed"): the same code addresses the gather vector where the step before streamed it -- the
// history's level, the log-beta row -- and y in a spill row of the slot.  It takes no dynamic LDS.  Same operands, same bits.
//
// Every value is formed by the functions of num_device.h on the operands and in the order of the windowed kernel: on a
// supervision both serve, the two give the same bits in every output.  No atomics, fixed orders: a sequence's bits do not
// depend on its batch.  A ragged handle's padding frames are not touched.  The staged hand-over (NumParams::staged) and the
// scatter are the windowed kernel's.
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"

namespace tc {

constexpr int kWideThreads = 1024;

// E, RAGGED: as num_windowed_kernel's.  SLOT: the gather vector and y are addressed in the pool slot, not in LDS.
template <typename E, bool RAGGED, bool SLOT>
__global__ __launch_bounds__(kWideThreads) void num_wide_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
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
  // this sequence's rows of the slot (num_wide_seq_doubles): log-beta [2][W], occupations [win_arcs], y spill [win_uniq]
  double *beta_row = p.wide_rows + (int64_t)q * p.wide_stride;
  float *occ = reinterpret_cast<float *>(beta_row + 2 * (size_t)W);
  double *gather_lds = reinterpret_cast<double *>(lds_raw);                        // [W]       (LDS form)
  float *ylp = SLOT ? occ + p.win_arcs : reinterpret_cast<float *>(gather_lds + W);  // [win_uniq]
  // the gather vector of a step: `row` (n entries, written before the last barrier) where it lies, or its copy in LDS
  auto gather_from = [&](const double *row, int n) __attribute__((always_inline)) {
    if (SLOT) return row;
    for (int i = tid; i < n; i += kWideThreads) gather_lds[i] = row[i];
    return (const double *)gather_lds;
  };

  // ---- forward: level t -> level t + 1 ----
  if (tid == 0) hist[0] = 0.0;  // level 0 is the start state alone
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    for (int u = u0 + tid; u < u1; u += kWideThreads) ylp[u - u0] = num_load_y<E>(p, q, ub + u);
    const double *cur = gather_from(hist + s0, s1 - s0);
    __syncthreads();
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s1 + tid; st < s2; st += kWideThreads)
      hist[st] = num_state_log_sum(in_begin[st], in_begin[st + 1],
                                   [&](int i) __attribute__((always_inline)) { return in_arc[i]; }, score,
                                   [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
    __syncthreads();
  }
  const int f0 = level[T], f1 = level[T + 1];
  {
    const double *last = gather_from(hist + f0, f1 - f0);
    __syncthreads();
    if (tid == 0) {
      const double tot = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
      tot_sh = tot;
      p.seq_logprob[q] = tot;
    }
  }
  if (!want_beta) return;
  for (int st = f0 + tid; st < f1; st += kWideThreads) beta_row[(size_t)(T & 1) * W + st - f0] = (double)final_logw[st];
  __syncthreads();
  const double tot = tot_sh;

  // ---- backward: level t + 1 -> level t, and the posteriors of frame t ----
  const int *uniq_begin = p.t.uniq_begin + ub + q;
  const int *uniq_arc = p.t.uniq_arc + ab;
  for (int t = T - 1; t >= 0; --t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    // (the posteriors of frame t + 1 may still be summing `occ`: they read neither y nor the gather vector)
    for (int u = u0 + tid; u < u1; u += kWideThreads) ylp[u - u0] = num_load_y<E>(p, q, ub + u);
    const double *nxt = gather_from(beta_row + (size_t)((t + 1) & 1) * W, s2 - s1);
    __syncthreads();
    double *cur = beta_row + (size_t)(t & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s0 + tid; st < s1; st += kWideThreads)
      cur[st - s0] = num_state_log_sum(out_begin[st], out_begin[st + 1], [](int a) __attribute__((always_inline)) { return a; },
                                       score, [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1]; });
    for (int a = a0 + tid; a < a1; a += kWideThreads)
      occ[a - a0] = num_occupation(hist[arc_src[a]], score(a), nxt[arc_dst[a] - s1], tot);
    __syncthreads();
    for (int u = u0 + tid; u < u1; u += kWideThreads)
      p.t.stage[ub + u] = num_posterior(p, uniq_arc, uniq_begin[u], uniq_begin[u + 1],
                                        [&](int a) __attribute__((always_inline)) { return occ[a - a0]; });
  }
  if (p.staged) return;  // beside the denominator: launch_num_scatter adds the posteriors once deriv is written
  __syncthreads();
  // scatter, as num_scatter_kernel: entry u on lane u mod kNumScatterLanes (the stage writes above are this workgroup's
  // own, ordered before these reads by the barrier)
  double xo = 0.0;
  if (tid < kNumScatterLanes)
    for (int u = tid; u < nu; u += kNumScatterLanes) num_scatter_one<E>(p, q, ub + u, p.t.stage[ub + u], xo);
  if (p.seq_xent) seq_xent_sum(xo, p.seq_xent + q, tid);
}

namespace {
template <typename E, bool RAGGED, bool SLOT>
int launch_wide(const NumParams &p, size_t lds, hipStream_t stream) {
  TC_HIP_CHECK(allow_dynamic_lds((const void *)num_wide_kernel<E, RAGGED, SLOT>, lds));
  hipLaunchKernelGGL((num_wide_kernel<E, RAGGED, SLOT>), dim3(p.S), dim3(kWideThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_wide(const NumParams &p, bool slot, hipStream_t stream) {
  const size_t lds = slot ? 0 : num_wide_lds_bytes(p.win_states, p.win_uniq);
  if (p.seq_frames) {  // a ragged supervision: its own level offsets come with its lengths
    if (!p.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
    return slot ? launch_wide<E, true, true>(p, lds, stream) : launch_wide<E, true, false>(p, lds, stream);
  }
  return slot ? launch_wide<E, false, true>(p, lds, stream) : launch_wide<E, false, false>(p, lds, stream);
}
}  // namespace

int launch_num_wide(const NumParams &p, hipStream_t stream) {
  // (a handle that reached the device before "force_num_wide" was set took a slot without the rows: stage_locked)
  if (!p.wide_rows || !p.t.alpha_hist || !p.t.frame_uniq) return TC_ERR_UNSUPPORTED;
  const bool slot = num_wide_slot_form(p.win_states, p.win_uniq);
  count_launch(kCntNumWide);
  if (p.elem == TC_DTYPE_BF16) return launch_wide<__hip_bfloat16>(p, slot, stream);
  if (p.elem == TC_DTYPE_F16) return launch_wide<__half>(p, slot, stream);
  return launch_wide<float>(p, slot, stream);
}

}  // namespace tc
