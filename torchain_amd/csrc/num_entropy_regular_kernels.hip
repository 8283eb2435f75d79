// Entropy of a REGULAR (time-unfolded) supervision's path posterior and its gradient, for gfx950
// (tc_supervision_path_entropy_regular).  The quantity is num_entropy_kernels.hip's: paths are the start-to-final paths of a
// sequence's acceptor, each exactly T arcs long, log W(path) = sum_t (y_t(pdf_t) + logw_t) - final cost, H = log Z - E[log W]
// and dH / dy_t(j) = -(E[log W 1(pdf j at t)] - E[log W] gamma_t(j)); it is carried in the log domain and in MEAN form, a
// state holding beside log alpha the posterior mean Abar of its prefixes' log W (double), so nothing is centred.
//
// What differs is the walk.  The acceptor has one level per frame: a state lives in one level, the arcs leaving level t are
// one range of arc ids and the unique (frame, pdf) entries of frame t one range of entries (NumTables' level bounds, CSRs and
// frame_uniq, as num_windowed_kernel and the best-path kernel walk them).  So every state is visited once per direction, two
// adjacent levels are all the recursion needs on chip, and the history is one 16-byte pair per state for the WHOLE sequence.
//
// One workgroup of 256 threads owns one sequence; one launch.  LDS, sized by the batch's widest level (num_ent_regular_lds_bytes):
//   pp   [2][W] double2  the ping-pong levels: (log alpha, Abar) forward, (log beta, Bbar) backward
//   ah   [W]    double2  the current level's (log alpha, Abar), back from the history            (GRAD)
//   ylp  [U]    float    y per unique entry of the frame
//   term [A]    float    the gradient terms of the arcs leaving the level                        (GRAD)
// forward, t = 0 .. T - 1 : stage frame t's y (registers -> LDS; the registers then fetch frame t + 1), barrier; thread k
//   takes the states s1 + k, s1 + k + 256, ... of level t + 1: log alpha by num_device.h's num_state_log_sum on the numerator's
//   operands in its order -- log Z has the numerator's bits -- then Abar as the double sum of share * (Abar(src) + r) over the
//   double sum of the shares, share = the float32 exp of (log alpha(src) + r - log alpha); a share of exactly 0 stays out.
//   With GRAD the pair goes to the workspace in one 16-byte store.  Barrier.
//   log Z by num_total and E[log W] by the same shares over the final states: one lane, as in the numerator.
// backward, t = T - 1 .. 0: stage frame t's y (fetching frame t - 1) and level t's history pairs, barrier; the states of
//   level t form (log beta, Bbar) from level t + 1's over their out-arcs, the arcs leaving the level (arc a0 + k, + 256, ...)
//   their terms occ (Abar(src) + r + Bbar(dst) - E[log W]), occ = num_occupation's; barrier; entry u0 + k, + 256, ... sums its
//   arcs' terms in uniq_arc order and makes ONE store of -grad_output * sum (the product in double, rounded once).
// Two barriers a level in each direction.  The level tables are read from global memory (L2), as in num_windowed_kernel.
//
// The gradient buffer is defined everywhere: the workgroup first writes +0 into every element of its sequence, padding
// frames included, and the backward pass stores over it behind the forward pass's barriers.  A sequence without a path
// (log Z = -inf: logprob -inf, entropy NaN) or with a NaN / +-inf among the y it reads (both NaN; found where y is staged)
// returns before the backward pass.  Only the caller's workspace is written: the supervision's pool slot is read for its
// tables.  No atomics, every sum in a fixed order, nothing depends on blockIdx but the sequence's own data.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"
#include "num_entropy_device.h"

namespace tc {

namespace {

constexpr int kEntRegThreads = 256;
constexpr int kEntRegYRegs = 2;  // unique entries of a frame a thread fetches a frame ahead; further ones load where staged

}  // namespace

template <typename El, bool RAGGED, bool GRAD>
__global__ __launch_bounds__(kEntRegThreads) void num_entropy_regular_kernel(const NumEntParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double tot_sh[2];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, W = n.win_states;
  double2 *pp = reinterpret_cast<double2 *>(lds_raw);                     // [2][W]
  double2 *ah = pp + 2 * W;                                               // [W] (GRAD)
  float *ylp = reinterpret_cast<float *>(pp + (GRAD ? 3 : 2) * (size_t)W);  // [win_uniq]
  float *term = ylp + n.win_uniq;                                         // [win_arcs] (GRAD)

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

  if (GRAD) {  // +0 everywhere; the backward pass stores over it behind the barriers of the forward pass
    if (n.y_bct) {
      const int64_t base = (int64_t)q * n.P * n.T, cnt = (int64_t)n.P * n.T;
      for (int64_t i = tid; i < cnt; i += kEntRegThreads) entr_store<El>(p.grad, base + i, 0.f);
    } else {
      float *g = reinterpret_cast<float *>(p.grad);
      for (int t = 0; t < n.T; ++t) {
        float *row = g + ((int64_t)t * n.S + q) * p.grad_stride;
        for (int j = tid; j < n.P; j += kEntRegThreads) row[j] = 0.f;
      }
    }
  }

  // y of a frame's unique entries: entry u0 + tid + r * 256 waits in register r from a frame ahead
  float ynx[kEntRegYRegs];
  bool bad = false;
  auto fetch = [&](int t) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kEntRegYRegs; ++r) {
      const int u = u0 + tid + r * kEntRegThreads;
      if (u < u1) ynx[r] = num_load_y<El>(n, q, ub + u);
    }
  };
  // frame t's y into ylp; `ahead` (-1: none) is the frame the registers fetch next
  auto stage_y = [&](int t, int ahead) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kEntRegYRegs; ++r) {
      const int u = u0 + tid + r * kEntRegThreads;
      if (u < u1) {
        ylp[u - u0] = ynx[r];
        bad |= !(ynx[r] - ynx[r] == 0.f);
      }
    }
    for (int u = u0 + tid + kEntRegYRegs * kEntRegThreads; u < u1; u += kEntRegThreads) {
      const float y = num_load_y<El>(n, q, ub + u);
      ylp[u - u0] = y;
      bad |= !(y - y == 0.f);
    }
    if (ahead >= 0) fetch(ahead);
  };

  // ---- forward: level t -> level t + 1 ----
  if (tid == 0) {
    pp[0] = make_double2(0.0, 0.0);  // level 0 is the start state alone
    if (GRAD) hist[0] = make_double2(0.0, 0.0);
  }
  fetch(0);
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t];
    stage_y(t, t + 1 < T ? t + 1 : -1);
    __syncthreads();
    const double2 *cur = pp + (t & 1) * W;
    double2 *nxt = pp + ((t + 1) & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    auto arc_at = [&](int i) __attribute__((always_inline)) { return in_arc[i]; };
    for (int st = s1 + tid; st < s2; st += kEntRegThreads) {
      const int i0 = in_begin[st], i1 = in_begin[st + 1];
      const double la = num_state_log_sum(i0, i1, arc_at, score,
                                          [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0].x; });
      const double ma = entr_state_mean(i0, i1, la, arc_at, score,
                                        [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
      nxt[st - s1] = make_double2(la, ma);
      if (GRAD) hist[st] = make_double2(la, ma);
    }
    __syncthreads();
  }

  // log Z (the numerator's num_total) and E[log W] over the final states
  const int f0 = level[T], f1 = level[T + 1];
  if (tid == 0) {
    const double2 *last = pp + (T & 1) * W;
    const double tot = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0].x; });
    tot_sh[0] = tot;
    tot_sh[1] = entr_final_mean(f0, f1, final_logw, tot, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
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
  for (int st = f0 + tid; st < f1; st += kEntRegThreads) {
    const double fl = (double)final_logw[st];
    pp[(T & 1) * W + st - f0] = make_double2(fl, fl > -INFINITY ? fl : 0.0);
  }
  // (the registers hold frame T - 1's y: the forward pass's last fetch)
  for (int t = T - 1; t >= 0; --t) {
    const int s0 = level[t], s1 = level[t + 1];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    stage_y(t, t > 0 ? t - 1 : -1);
    for (int st = s0 + tid; st < s1; st += kEntRegThreads) ah[st - s0] = hist[st];
    __syncthreads();
    const double2 *nxt = pp + ((t + 1) & 1) * W;
    double2 *cur = pp + (t & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return ylp[arc_uniq[a] - u0] + arc_logw[a]; };
    auto arc_at = [](int a) __attribute__((always_inline)) { return a; };
    for (int st = s0 + tid; st < s1; st += kEntRegThreads) {
      const int i0 = out_begin[st], i1 = out_begin[st + 1];
      const double lb = num_state_log_sum(i0, i1, arc_at, score,
                                          [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1].x; });
      const double mb = entr_state_mean(i0, i1, lb, arc_at, score,
                                        [&](int a) __attribute__((always_inline)) { return nxt[arc_dst[a] - s1]; });
      cur[st - s0] = make_double2(lb, mb);
    }
    for (int a = a0 + tid; a < a1; a += kEntRegThreads) {
      const float sc = score(a);
      const double2 h = ah[arc_src[a] - s0], b = nxt[arc_dst[a] - s1];
      const float occ = num_occupation(h.x, sc, b.x, logz);  // (exp(-inf) = 0: an arc no path takes)
      term[a - a0] = occ > 0.f ? (float)((double)occ * (h.y + (double)sc + b.y - elw)) : 0.f;
    }
    __syncthreads();
    for (int u = u0 + tid; u < u1; u += kEntRegThreads) {
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
int launch_entr(const NumEntParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumEntParams) = num_entropy_regular_kernel<El, RAGGED, GRAD>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kEntRegThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename El>
int launch_entr(const NumEntParams &p, size_t lds, hipStream_t stream) {
  if (p.n.seq_frames) return p.grad ? launch_entr<El, true, true>(p, lds, stream) : launch_entr<El, true, false>(p, lds, stream);
  return p.grad ? launch_entr<El, false, true>(p, lds, stream) : launch_entr<El, false, false>(p, lds, stream);
}

}  // namespace

int launch_num_entropy_regular(const NumEntParams &p, hipStream_t stream) {
  if (p.n.t.e2e || !p.entropy || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (p.n.seq_frames && !p.n.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
  if (p.grad && !p.hist) return TC_ERR_WORKSPACE;
  if (!p.n.t.frame_uniq || !num_ent_regular_fits(p.n.win_states, p.n.win_arcs, p.n.win_uniq)) return TC_ERR_UNSUPPORTED;
  const size_t lds = num_ent_regular_lds_bytes(p.n.win_states, p.n.win_arcs, p.n.win_uniq, p.grad != nullptr);
  count_launch(kCntNumEntropyRegular);
  if (p.n.elem == TC_DTYPE_BF16) return launch_entr<__hip_bfloat16>(p, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_entr<__half>(p, lds, stream);
  return launch_entr<float>(p, lds, stream);
}

}  // namespace tc
