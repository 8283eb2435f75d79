// Entropy of a REGULAR supervision's path posterior and its gradient for handles with time levels of any width, for gfx950
// (tc_supervision_path_entropy_regular on a handle of tc_supervision_allow_wide_levels whose widest level is beyond
// num_entropy_regular_kernels.hip's LDS, or under "force_num_entropy_wide").  The quantity, the semiring and every formula are
// that kernel's: the log domain in MEAN form, a state carrying (log alpha, Abar) as one double2, H = log Z - E[log W], an
// arc's gradient term occ * (Abar(src) + r + Bbar(dst) - E[log W]).  What differs is the walk, which is num_wide_kernels.hip's.
//
// ONE WORKGROUP OF 1024 THREADS (16 waves) owns a sequence and walks its levels, two barriers a level in each direction.
// What a step addresses at random is one per-state vector of pairs, the GATHER VECTOR: (log alpha, Abar) of level t, gathered
// through arc_src by the states of level t + 1 (forward); (log beta, Bbar) of level t + 1, gathered through arc_dst by the
// states and the leaving arcs of level t (backward).  It (16 bytes a state) and y of the frame's unique entries (4 bytes an
// entry) are all that LDS holds.  Everything else streams through the CALLER'S WORKSPACE with unit-stride accesses:
//   (log alpha, Abar) of every state -> the history, one double2 per state of the handle (GRAD); the backward pass reads an
//                                       arc's source pair from it where it lies (arcs are sorted by source: nearly unit stride);
//   per sequence (num_ent_wide_seq_doubles): two level-sized rows of pairs, ping-pong -- (log beta, Bbar) with GRAD, (log alpha,
//                                       Abar) for the value alone, which needs no history --; with GRAD one float row of the
//                                       leaving arcs' terms, read back by the entry sums after the barrier; a y spill row.
// After the barrier that ends a step, the row it wrote is loaded into LDS as the next step's gather vector.
//
// SLOT form (a level beyond 16 * ceil2(states) + 4 * ceil4(frame's entries) + 2048 <= 163840, about 10000 states; or
// "force_num_entropy_wide_streamed"): the same code addresses the gather vector where the step before streamed it -- the
// history's level or a ping-pong row -- and y in the spill row.  It takes no dynamic LDS.  Same operands, same order, same bits.
//
// The regular kernel's contract is kept: the workgroup first writes +0 into every gradient element of its sequence, padding
// included; a NaN or an infinity among the y it reads gives (NaN, NaN), a sequence without a path (NaN, -inf), both return
// before the backward pass, the others keep their bits.  log alpha, log beta, log Z and the occupations are num_device.h's on the
// numerator's operands in its order, the means num_entropy_device.h's: logprob has the numerator's bits, and on a handle both
// entropy kernels serve every output has the regular kernel's.  No atomics, fixed orders, nothing depends on blockIdx but the
// sequence's own data.  Only the workspace is written: the supervision's pool slot is read for its tables.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"
#include "num_entropy_device.h"

namespace tc {

namespace {
constexpr int kEntWideThreads = 1024;
}

// El, RAGGED, GRAD: as num_entropy_regular_kernel's.  SLOT: the gather vector and y are addressed in the workspace, not in LDS.
template <typename El, bool RAGGED, bool GRAD, bool SLOT>
__global__ __launch_bounds__(kEntWideThreads) void num_entropy_wide_kernel(const NumEntParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double tot_sh[2];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, W = n.win_states;
  const int T = RAGGED ? ragged_frames(n.seq_frames, q, n.T) : n.T;
  const int64_t lo = RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(n.seq_level_off[q]) : (int64_t)q * (T + 2);
  const int sb = n.t.seq_state_off[q];
  const int ab = n.t.seq_arc_off[q];
  const int ub = n.t.seq_uniq_off[q];
  const int *level = n.t.level_begin + lo;
  const int *frame_uniq = n.t.frame_uniq + (RAGGED ? lo - q : (int64_t)q * (T + 1));
  const int *out_begin = n.t.out_begin + sb + q;
  const int *in_begin = n.t.in_begin + sb + q;
  const int *in_arc = n.t.in_arc + ab;
  const int *arc_src = n.t.arc_src + ab, *arc_dst = n.t.arc_dst + ab, *arc_uniq = n.t.arc_uniq + ab;
  const float *arc_logw = n.t.arc_logw + ab;
  const float *final_logw = n.t.final_logw + sb;
  double2 *hist = GRAD ? reinterpret_cast<double2 *>(p.hist) + sb : nullptr;  // one pair per state of the handle
  // this sequence's rows of the workspace (num_ent_wide_seq_doubles): pairs [2][W], terms [win_arcs] (GRAD), y spill [win_uniq]
  double2 *row = reinterpret_cast<double2 *>(n.wide_rows + (int64_t)q * n.wide_stride);
  float *term = reinterpret_cast<float *>(row + 2 * (size_t)W);
  double2 *gather_lds = reinterpret_cast<double2 *>(lds_raw);  // [W]  (LDS form)
  float *ylp = SLOT ? term + (GRAD ? n.win_arcs : 0) : reinterpret_cast<float *>(gather_lds + W);  // [win_uniq]
  // the gather vector of a step: `from` (cnt pairs, written before the last barrier) where it lies, or its copy in LDS
  auto gather_from = [&](const double2 *from, int cnt) __attribute__((always_inline)) {
    if (SLOT) return from;
    for (int i = tid; i < cnt; i += kEntWideThreads) gather_lds[i] = from[i];
    return (const double2 *)gather_lds;
  };
  // where level t's (log alpha, Abar) stream to, entry st - level[t]: the history, or for the value alone a ping-pong row
  auto alpha_level = [&](int t, int s_t) __attribute__((always_inline)) { return GRAD ? hist + s_t : row + (size_t)(t & 1) * W; };

  if (GRAD) {  // +0 everywhere; the backward pass stores over it behind the barriers of the forward pass
    if (n.y_bct) {
      const int64_t base = (int64_t)q * n.P * n.T, cnt = (int64_t)n.P * n.T;
      for (int64_t i = tid; i < cnt; i += kEntWideThreads) entr_store<El>(p.grad, base + i, 0.f);
    } else {
      float *g = reinterpret_cast<float *>(p.grad);
      for (int t = 0; t < n.T; ++t) {
        float *grow = g + ((int64_t)t * n.S + q) * p.grad_stride;
        for (int j = tid; j < n.P; j += kEntWideThreads) grow[j] = 0.f;
      }
    }
  }

  bool bad = false;
  // frame t's y per unique entry into ylp (LDS, or the spill row)
  auto stage_y = [&](int u0, int u1) __attribute__((always_inline)) {
    for (int u = u0 + tid; u < u1; u += kEntWideThreads) {
      const float y = num_load_y<El>(n, q, ub + u);
      ylp[u - u0] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward: level t -> level t + 1 ----
  if (tid == 0) alpha_level(0, 0)[0] = make_double2(0.0, 0.0);  // level 0 is the start state alone
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    stage_y(u0, u1);
    const double2 *cur = gather_from(alpha_level(t, s0), s1 - s0);
    __syncthreads();
    double2 *nxt = alpha_level(t + 1, s1);
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    auto arc_at = [&](int i) __attribute__((always_inline)) { return in_arc[i]; };
    for (int st = s1 + tid; st < s2; st += kEntWideThreads) {
      const int i0 = in_begin[st], i1 = in_begin[st + 1];
      const double la = num_state_log_sum(i0, i1, arc_at, score,
                                          [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0].x; });
      const double ma = entr_state_mean(i0, i1, la, arc_at, score,
                                        [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
      nxt[st - s1] = make_double2(la, ma);
    }
    __syncthreads();
  }

  // log Z (the numerator's num_total) and E[log W] over the final states: one lane, as in the numerator
  const int f0 = level[T], f1 = level[T + 1];
  {
    const double2 *last = gather_from(alpha_level(T, f0), f1 - f0);
    __syncthreads();
    if (tid == 0) {
      const double tot = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0].x; });
      tot_sh[0] = tot;
      tot_sh[1] = entr_final_mean(f0, f1, final_logw, tot, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
    }
  }
  const bool some_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  const double logz = tot_sh[0], elw = tot_sh[1];
  const bool any_bad = some_bad || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  const bool ok = !any_bad && logz > -INFINITY;
  if (tid == 0) {
    p.logprob[q] = any_bad ? (double)NAN : logz;
    p.entropy[q] = ok ? logz - elw : (double)NAN;
  }
  if (!GRAD || !ok) return;

  // ---- backward: level t + 1 -> level t, and the gradient of frame t ----
  const double scale = p.grad_output ? p.grad_output[q] : 1.0;
  const int *uniq_begin = n.t.uniq_begin + ub + q;
  const int *uniq_arc = n.t.uniq_arc + ab;
  for (int st = f0 + tid; st < f1; st += kEntWideThreads) {
    const double fl = (double)final_logw[st];
    row[(size_t)(T & 1) * W + st - f0] = make_double2(fl, fl > -INFINITY ? fl : 0.0);
  }
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    // (the entries of frame t + 1 may still be summing `term`: they read neither y nor the gather vector)
    stage_y(u0, u1);
    const double2 *nxt = gather_from(row + (size_t)((t + 1) & 1) * W, s2 - s1);
    __syncthreads();
    double2 *cur = row + (size_t)(t & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    auto arc_at = [](int a) __attribute__((always_inline)) { return a; };
    for (int st = s0 + tid; st < s1; st += kEntWideThreads) {
      const int i0 = out_begin[st], i1 = out_begin[st + 1];
      const double lb = num_state_log_sum(i0, i1, arc_at, score,
                                          [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1].x; });
      const double mb = entr_state_mean(i0, i1, lb, arc_at, score,
                                        [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1]; });
      cur[st - s0] = make_double2(lb, mb);
    }
    for (int a = a0 + tid; a < a1; a += kEntWideThreads) {
      const float sc = score(a);
      const double2 h = hist[arc_src[a]], b = nxt[arc_dst[a] - s1];
      const float occ = num_occupation(h.x, sc, b.x, logz);  // (exp(-inf) = 0: an arc no path takes)
      term[a - a0] = occ > 0.f ? (float)((double)occ * (h.y + (double)sc + b.y - elw)) : 0.f;
    }
    __syncthreads();
    for (int u = u0 + tid; u < u1; u += kEntWideThreads) {
      float g = 0.f;
      for (int i = uniq_begin[u]; i < uniq_begin[u + 1]; ++i) g += term[uniq_arc[i] - a0];
      const float v = (float)(-scale * (double)g);
      const int pdf = n.t.uniq_pdf[ub + u];
      if (n.y_bct)
        entr_store<El>(p.grad, ((int64_t)q * n.P + pdf) * n.T + t, v);
      else
        reinterpret_cast<float *>(p.grad)[((int64_t)t * n.S + q) * p.grad_stride + pdf] = v;
    }
  }
}

namespace {

template <typename El, bool RAGGED, bool GRAD>
int launch_entw(const NumEntParams &p, bool slot, hipStream_t stream) {
  const size_t lds = slot ? 0 : num_ent_wide_lds_bytes(p.n.win_states, p.n.win_uniq);
  void (*kernel)(const NumEntParams) =
      slot ? num_entropy_wide_kernel<El, RAGGED, GRAD, true> : num_entropy_wide_kernel<El, RAGGED, GRAD, false>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kEntWideThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename El>
int launch_entw(const NumEntParams &p, bool slot, hipStream_t stream) {
  if (p.n.seq_frames) return p.grad ? launch_entw<El, true, true>(p, slot, stream) : launch_entw<El, true, false>(p, slot, stream);
  return p.grad ? launch_entw<El, false, true>(p, slot, stream) : launch_entw<El, false, false>(p, slot, stream);
}

}  // namespace

int launch_num_entropy_wide(const NumEntParams &p, bool slot, hipStream_t stream) {
  if (p.n.t.e2e || !p.entropy || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (p.n.seq_frames && !p.n.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
  if (!p.n.wide_rows || p.n.wide_stride <= 0 || (p.grad && !p.hist)) return TC_ERR_WORKSPACE;
  if (!p.n.t.frame_uniq) return TC_ERR_UNSUPPORTED;
  if (!slot && !num_ent_wide_lds_fits(p.n.win_states, p.n.win_uniq)) return TC_ERR_UNSUPPORTED;
  count_launch(kCntNumEntropyWide);
  if (p.n.elem == TC_DTYPE_BF16) return launch_entw<__hip_bfloat16>(p, slot, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_entw<__half>(p, slot, stream);
  return launch_entw<float>(p, slot, stream);
}

}  // namespace tc
