// Arc occupations of a REGULAR (time-unfolded) supervision, for gfx950 (tc_supervision_arc_posteriors_regular): per sequence
// the posterior probability of every arc of its acceptor under the numerator's distribution over the start-to-final paths,
// and the probability that the path ends in each state of the last level,
//   arcs(a)   = exp(log alpha_t(src_a) + term(a) - log Z),  term(a) = (y_t(pdf_a) + logw_a) + log beta_{t+1}(dst_a),
//   finals(i) = exp(log alpha_T(i) + final_logw(i) - log Z):
// d log Z / d(-cost) and d log Z / d(-final cost).  The acceptor has one level per frame (NumTables: level_begin, the CSRs,
// frame_uniq, as num_windowed_kernel walks them), so an arc is taken at ONE frame: there is nothing to accumulate over
// frames, num_arc_post_kernels.hip's arc-stationary registers have no use, and an occupation is stored once.
//
// One workgroup of 256 threads owns one sequence; one launch.  LDS, laid out by the handle's widest level (L states, A arcs
// leaving a level, U unique entries of a frame; num_arc_regular_lds_bytes):
//   B    [2][L] double  log beta of two adjacent levels, ping-pong (the forward pass: log alpha)
//   AL   [L]    double  log alpha of the current level, back from the history
//   TERM [A]    double  the terms of the arcs leaving the level             (resident form; SPILL: in the workspace)
//   Y    [U]    float   y per unique entry of the frame
// forward, t = 0 .. T - 1: the level-windowed numerator's recursion through num_device.h (num_load_y, num_state_log_sum,
//   num_total) on its operands in its order, so logprob is the numerator's log Z bit for bit.  log alpha of every state goes
//   to the CALLER'S workspace, 8 bytes a state of the handle; the pool slot's alpha_hist and stage are not touched.
// backward, t = T - 1 .. 0, ARC-PARALLEL in two phases with two barriers a level:
//   arcs   : thread k takes the arcs a0 + k, a0 + k + 256, ... leaving level t.  It forms the arc's term -- the y gather and
//            the numerator's one float32 sum y + logw once, for both uses -- stores it at the arc's position in TERM and
//            stores the occupation, the float32 exp of (log alpha_t(src) - log Z) + term widened to double, at the arc's
//            place in the output.
//   states : the owner of state i of level t takes log beta_t(i) over its contiguous slice [out_begin[i], out_begin[i + 1])
//            of TERM: maximum, float32 sum of exp, double log.  (The windowed numerator forms every arc's score twice, once
//            per state list and once per occupation; level 0 needs no log beta.)
// A level ahead, into registers, behind the arcs phase's arithmetic: the next frame's y (2 entries a thread), the next
// level's history (2 states a thread) and up to four arc records a thread (dst, uniq, logw, src); whatever a level has
// beyond that loads where it is used.
//
// SPILL form (a level whose arcs do not fit beside the rest, or "force_num_arc_post_regular_spill"): TERM lives in the
// workspace, 8 * max_level_arcs bytes a sequence.  A term stored by one thread is loaded by others of the SAME workgroup one
// barrier later, which the barrier's workgroup-scope release and acquire order (the waves of a workgroup share their CU's
// vector L1; num_entropy_large_kernels.hip orders its mean rows the same way).  Same operands in the same orders: the
// resident form's bits.
//
// No atomics, every sum in table order, nothing depends on blockIdx but the sequence's own data.  Failure: no path (log Z =
// -inf: logprob -inf) or a NaN / +-inf among the y the sequence reads (logprob NaN; found where y is staged, not left to the
// recursion).  Either way the workgroup writes +0 into all its arcs and finals and returns before the backward pass.
// Otherwise every arc and every final is stored once.  A ragged sequence walks its own T_s levels.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"

namespace tc {

namespace {

constexpr int kArcRegThreads = 256;
constexpr int kArcRegYRegs = 2;     // unique entries of a frame a thread fetches a frame ahead
constexpr int kArcRegHistRegs = 2;  // states of a level whose log alpha a thread fetches a level ahead
constexpr int kArcRegArcRegs = 4;   // arc records a thread fetches a level ahead

// the workgroup's barrier: release of this wave's global and LDS stores, barrier, acquire (what __syncthreads() is)
__device__ __forceinline__ void arcr_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// log-sum over term[b, e): the maximum, the float32 sum of the float32 exp of the double differences, a double log
__device__ __forceinline__ double arcr_logsum(const double *term, int b, int e) {
  double mx = -INFINITY;
  for (int a = b; a < e; ++a) mx = fmax(mx, term[a]);
  if (!(mx > -INFINITY)) return mx;
  float sum = 0.f;
  for (int a = b; a < e; ++a) sum += __expf((float)(term[a] - mx));
  return mx + log((double)sum);
}

}  // namespace

template <typename El, bool RAGGED, bool SPILL>
__global__ __launch_bounds__(kArcRegThreads) void num_arc_post_regular_kernel(const NumArcRegParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double tot_sh;

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, W = n.win_states;
  double *B = reinterpret_cast<double *>(lds_raw);            // [2][W]
  double *AL = B + 2 * W;                                     // [W]
  double *TERM = SPILL ? p.terms + (int64_t)q * p.term_stride : AL + W;  // [win_arcs]
  float *Y = reinterpret_cast<float *>(AL + W + (SPILL ? 0 : n.win_arcs));  // [win_uniq]

  const int T = RAGGED ? ragged_frames(n.seq_frames, q, n.T) : n.T;
  const int64_t lo = RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(n.seq_level_off[q]) : (int64_t)q * (T + 2);
  const int sb = n.t.seq_state_off[q];
  const int ab = n.t.seq_arc_off[q], narc = n.t.seq_arc_off[q + 1] - ab;
  const int ub = n.t.seq_uniq_off[q];
  const int *level = n.t.level_begin + lo;
  const int *frame_uniq = n.t.frame_uniq + (RAGGED ? lo - q : (int64_t)q * (T + 1));
  const int *out_begin = n.t.out_begin + sb + q;
  const int *in_begin = n.t.in_begin + sb + q;
  const int *in_arc = n.t.in_arc + ab;
  const int *arc_src = n.t.arc_src + ab, *arc_dst = n.t.arc_dst + ab, *arc_uniq = n.t.arc_uniq + ab;
  const float *arc_logw = n.t.arc_logw + ab;
  const float *final_logw = n.t.final_logw + sb;
  double *hist = p.hist + sb;  // log alpha of every state of the sequence
  double *arcs = p.arcs + ab, *finals = p.finals + sb;

  // y of a frame's unique entries: entry u0 + tid + r * 256 waits in register r from a frame ahead
  float ynx[kArcRegYRegs] = {};
  bool bad = false;
  auto fetch_y = [&](int t) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kArcRegYRegs; ++r) {
      const int u = u0 + tid + r * kArcRegThreads;
      if (u < u1) ynx[r] = num_load_y<El>(n, q, ub + u);
    }
  };
  auto stage_y = [&](int t) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kArcRegYRegs; ++r) {
      const int u = u0 + tid + r * kArcRegThreads;
      if (u < u1) {
        Y[u - u0] = ynx[r];
        bad |= !(ynx[r] - ynx[r] == 0.f);
      }
    }
    for (int u = u0 + tid + kArcRegYRegs * kArcRegThreads; u < u1; u += kArcRegThreads) {
      const float y = num_load_y<El>(n, q, ub + u);
      Y[u - u0] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward: level t -> level t + 1, the windowed numerator's ----
  if (tid == 0) {
    B[0] = 0.0;  // level 0 is the start state alone
    hist[0] = 0.0;
  }
  fetch_y(0);
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t];
    stage_y(t);
    arcr_sync();
    if (t + 1 < T) fetch_y(t + 1);
    const double *cur = B + (t & 1) * W;
    double *nxt = B + ((t + 1) & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return Y[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s1 + tid; st < s2; st += kArcRegThreads) {
      const double v = num_state_log_sum(in_begin[st], in_begin[st + 1],
                                         [&](int i) __attribute__((always_inline)) { return in_arc[i]; }, score,
                                         [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
      nxt[st - s1] = v;
      hist[st] = v;
    }
    arcr_sync();
  }

  // log Z, the numerator's num_total: one lane
  const int f0 = level[T], f1 = level[T + 1];
  double *last = B + (T & 1) * W;
  if (tid == 0) tot_sh = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
  const bool some_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  const double logz = tot_sh;
  const bool any_bad = some_bad || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  if (tid == 0) p.logprob[q] = any_bad ? (double)NAN : logz;
  if (any_bad || !(logz > -INFINITY)) {
    const int nst = n.t.seq_state_off[q + 1] - sb;
    for (int a = tid; a < narc; a += kArcRegThreads) arcs[a] = 0.0;
    for (int st = tid; st < nst; st += kArcRegThreads) finals[st] = 0.0;
    return;
  }

  // ---- where the path ends, and log beta_T ----
  // (a thread reads log alpha_T of its own states before it overwrites them; the levels' first barrier orders the rest)
  for (int st = tid; st < f0; st += kArcRegThreads) finals[st] = 0.0;
  for (int st = f0 + tid; st < f1; st += kArcRegThreads) {
    const double fl = (double)final_logw[st];
    finals[st] = (double)__expf((float)((last[st - f0] + fl) - logz));  // (exp(-inf) = +0: a state that is not final)
    last[st - f0] = fl;
  }

  // ---- backward: level t + 1 -> level t, and the occupations of the arcs leaving level t ----
  // the next level's history and arc records wait in registers (the y registers hold frame T - 1: the forward pass's last)
  double hnx[kArcRegHistRegs] = {};
  int nd[kArcRegArcRegs] = {}, nu[kArcRegArcRegs] = {}, ns[kArcRegArcRegs] = {};
  float nw[kArcRegArcRegs] = {};
  auto fetch_level = [&](int t) __attribute__((always_inline)) {
    const int s0 = level[t], s1 = level[t + 1];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
#pragma unroll
    for (int r = 0; r < kArcRegHistRegs; ++r) {
      const int st = s0 + tid + r * kArcRegThreads;
      if (st < s1) hnx[r] = hist[st];
    }
#pragma unroll
    for (int r = 0; r < kArcRegArcRegs; ++r) {
      const int a = a0 + tid + r * kArcRegThreads;
      if (a < a1) {
        nd[r] = arc_dst[a];
        nu[r] = arc_uniq[a];
        nw[r] = arc_logw[a];
        ns[r] = arc_src[a];
      }
    }
  };
  fetch_level(T - 1);
  for (int t = T - 1; t >= 0; --t) {
    const int s0 = level[t], s1 = level[t + 1];
    const int a0 = out_begin[s0], a1 = out_begin[s1];
    const int u0 = frame_uniq[t];
    stage_y(t);
#pragma unroll
    for (int r = 0; r < kArcRegHistRegs; ++r) {
      const int st = s0 + tid + r * kArcRegThreads;
      if (st < s1) AL[st - s0] = hnx[r];
    }
    for (int st = s0 + tid + kArcRegHistRegs * kArcRegThreads; st < s1; st += kArcRegThreads) AL[st - s0] = hist[st];
    int cd[kArcRegArcRegs], cu[kArcRegArcRegs], cs[kArcRegArcRegs];
    float cw[kArcRegArcRegs];
#pragma unroll
    for (int r = 0; r < kArcRegArcRegs; ++r) {
      cd[r] = nd[r];
      cu[r] = nu[r];
      cw[r] = nw[r];
      cs[r] = ns[r];
    }
    arcr_sync();
    if (t > 0) {  // a level ahead, behind the arcs phase
      fetch_y(t - 1);
      fetch_level(t - 1);
    }
    const double *nxt = B + ((t + 1) & 1) * W;
    double *cur = B + (t & 1) * W;
    // one arc: its term into TERM, its occupation into the output
    auto arc = [&](int a, int dst, int uniq, float logw, int src) __attribute__((always_inline)) {
      const double term = (double)(Y[uniq - u0] + logw) + nxt[dst - s1];
      TERM[a - a0] = term;
      arcs[a] = (double)__expf((float)((AL[src - s0] - logz) + term));  // (exp(-inf) = +0: an arc no path takes)
    };
#pragma unroll
    for (int r = 0; r < kArcRegArcRegs; ++r) {
      const int a = a0 + tid + r * kArcRegThreads;
      if (a < a1) arc(a, cd[r], cu[r], cw[r], cs[r]);
    }
    for (int a = a0 + tid + kArcRegArcRegs * kArcRegThreads; a < a1; a += kArcRegThreads)
      arc(a, arc_dst[a], arc_uniq[a], arc_logw[a], arc_src[a]);
    if (t == 0) break;
    arcr_sync();  // (the terms' stores before their loads: see the head of the file)
    for (int st = s0 + tid; st < s1; st += kArcRegThreads) cur[st - s0] = arcr_logsum(TERM, out_begin[st] - a0, out_begin[st + 1] - a0);
  }
}

namespace {

template <typename El, bool SPILL>
int launch_arcr(const NumArcRegParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumArcRegParams) =
      p.n.seq_frames ? num_arc_post_regular_kernel<El, true, SPILL> : num_arc_post_regular_kernel<El, false, SPILL>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kArcRegThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <bool SPILL>
int launch_arcr(const NumArcRegParams &p, size_t lds, hipStream_t stream) {
  if (p.n.elem == TC_DTYPE_BF16) return launch_arcr<__hip_bfloat16, SPILL>(p, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_arcr<__half, SPILL>(p, lds, stream);
  return launch_arcr<float, SPILL>(p, lds, stream);
}

}  // namespace

int launch_num_arc_post_regular(const NumArcRegParams &p, bool spill, hipStream_t stream) {
  if (p.n.t.e2e || !p.arcs || !p.finals || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (p.n.seq_frames && !p.n.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
  if (!p.hist || (spill && !p.terms)) return TC_ERR_WORKSPACE;
  // (win_*: the widest level's counts, rounded as the rules round them)
  if (!p.n.t.frame_uniq || !num_arc_regular_fits(p.n.win_states, p.n.win_arcs, p.n.win_uniq, spill)) return TC_ERR_UNSUPPORTED;
  const size_t lds = num_arc_regular_lds_bytes(p.n.win_states, p.n.win_arcs, p.n.win_uniq, spill);
  count_launch(spill ? kCntNumArcPostRegularSpill : kCntNumArcPostRegular);
  return spill ? launch_arcr<true>(p, lds, stream) : launch_arcr<false>(p, lds, stream);
}

}  // namespace tc
