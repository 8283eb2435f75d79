// Arc occupations of an end-to-end supervision, for gfx950 (tc_supervision_arc_posteriors): per sequence the expected number
// of times each arc of its (cyclic) FST is taken under the posterior over the paths of exactly T arcs from the start state to
// a final state, and the probability that the path ends in each state,
//   arcs(a)   = sum_t exp(log alpha_t(src_a) + term_t(a) - log Z),  term_t(a) = (y_t(pdf_a) - cost_a) + log beta_{t+1}(dst_a),
//   finals(i) = exp(log alpha_T(i) - final(i) - log Z):
// d log Z / d(-cost) and d log Z / d(-final cost).  The numerator kernels form every one of these occupations each frame, add
// them up per pdf and drop them; here each is kept, by arc.
//
// One workgroup of 256 threads owns one sequence; one launch.
// Forward (both forms): num_e2e_kernel's, operand for operand -- threads own states and walk their in-arc lists,
// y + (-cost) one float32 sum, the float32 exp of a double difference, the float32 sum under a double log -- so log Z has the
// numerator's bits.  log alpha_t, t < T, goes to the CALLER'S workspace, 8 bytes a (frame, state): the supervision's pool slot
// is read for its tables alone, and what a training step finds there is what it left.
// Backward: ARC-STATIONARY.  Out-arc k of the sequence belongs to thread k % 256 for every frame.  A frame is two phases:
//   arcs   : the arc's owner forms term_t(a) into an array by arc position and adds the float32
//            exp((log alpha_t(src) - log Z) + term_t(a)) to the arc's double accumulator;
//   states : state i's owner takes log beta_t(i) as the log-sum (maximum, float32 sum of exp, double log) over the contiguous
//            slice [out_begin[i], out_begin[i + 1]) of that array.  Frame 0 needs no log beta_0.
// Two barriers a frame.  No atomics; an arc's accumulator takes its frames from T - 1 down to 0, a state's log-sum its arcs in
// table order; nothing depends on blockIdx but the sequence's own data, so a sequence's bits do not depend on its batch.
//
// RESIDENT form (every sequence within TC_E2E_MAX_STATES / _ARCS / _PDFS = 2048 / 8192 / 1024): the backward pass reads no
// table per frame.  A thread keeps in registers, read once from global memory:
//   its arcs' records, slot k / 256 of 32: one word (destination | source << 11 | distinct-pdf slot << 22; the source found
//   once from out_begin by arc_source), -cost, and the double accumulator;
//   its states' slice bounds, slot i / 256 of 8, and log alpha_{t-1} of those states, fetched from the workspace a frame ahead;
//   y_{t-1} of its distinct pdfs, slot of 4, fetched from the caller's tensor a frame ahead.
// LDS, laid out with the sequence's own sizes: [2][MS] log beta of two adjacent levels (the forward pass: log alpha) and [MS]
// log alpha_t as doubles, [MA] the terms as doubles, [MP] the frame's y as floats:
//   24 * ceil4(states) + 8 * ceil4(arcs) + 4 * ceil4(distinct pdfs) bytes, 48 + 64 + 4 = 116 KB at the limits, beside 2 KB for
//   the block reductions' slots (num_arc_lds_bytes, kNumArcStaticLds), of the 160.
// LARGE form (a handle with a sequence beyond those limits; tc_debug_set("force_num_arc_post_large", 1) for the others): log
// beta of two levels and the frame's y alone in LDS, 16 * ceil4(states) + 4 * ceil4(distinct pdfs) -- the any-size numerator's
// rule (e2e_large_fits), so whatever tc_supervision_create_e2e_any builds is served, with any number of arcs.  By arc in global
// memory: the terms and the sources (found once) in the workspace, the accumulators in the output itself (doubles there and
// here: nothing is rounded on the way); log alpha_t(src) is read from the history.  The arc's records come from the tables
// every frame, kGroup arcs' loads in flight at a time.  Same operands in the same orders: on a handle that fits both, the
// resident form's bits.  A term or a history row stored by one thread is loaded by others of the SAME workgroup one barrier
// later, which __syncthreads() orders (workgroup-scope release and acquire around the barrier; the waves of a workgroup share
// their CU's vector L1).
//
// Failure: no path of T arcs (log Z = -inf: logprob -inf), or a NaN / +-inf among the y the sequence reads in its valid
// frames (logprob NaN; found by the threads that stage y, not left to the recursion, where a max would drop a NaN).  Either
// way the workgroup writes +0 into all its arcs and finals and returns before the backward pass.  Otherwise every arc and every
// final is stored once.  A ragged sequence walks its own T_s frames: nothing at frames >= T_s is read.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kArcThreads = kE2eThreads;
constexpr int kArcPdfRegs = TC_E2E_MAX_PDFS / kArcThreads;      // 4: y a frame ahead
constexpr int kArcStateRegs = TC_E2E_MAX_STATES / kArcThreads;  // 8: slice bounds, log alpha a frame ahead
constexpr int kArcSlots = TC_E2E_MAX_ARCS / kArcThreads;        // 32: arc records and accumulators
constexpr int kGroup = 4;                                       // the large form's arcs in flight
static_assert(TC_E2E_MAX_STATES <= (1 << 11) && TC_E2E_MAX_PDFS <= (1 << 10), "an arc's record is one 32-bit word");
static_assert(TC_E2E_MAX_PDFS % kArcThreads == 0 && TC_E2E_MAX_STATES % kArcThreads == 0 && TC_E2E_MAX_ARCS % kArcThreads == 0,
              "register slots");

// the state whose out-arc slice holds arc k: the i with out_begin[i] <= k < out_begin[i + 1] (states without arcs are passed)
__device__ __forceinline__ int arc_source(const int32_t *out_begin, int n, int k) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (out_begin[mid + 1] <= k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// log-sum over term[b, e): the maximum, the float32 sum of the float32 exp of the double differences, a double log
__device__ __forceinline__ double arc_logsum(const double *term, int b, int e) {
  double mx = -INFINITY;
  for (int a = b; a < e; ++a) mx = fmax(mx, term[a]);
  if (!(mx > -INFINITY)) return mx;
  float sum = 0.f;
  for (int a = b; a < e; ++a) sum += __expf((float)(term[a] - mx));
  return mx + log((double)sum);
}

}  // namespace

template <typename El, bool RAGGED, bool LARGE>
__global__ __launch_bounds__(kArcThreads) void num_arc_post_kernel(const NumArcParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_x[4];
  __shared__ float red_s[4];
  __shared__ int red_bad[4];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? n.seq_frames[q] : n.T;
  const SeqView v = seq_view(n, q);  // (its hist and stage point into the pool slot: not used here)
  const int MS = (v.n + 3) & ~3, MA = (v.na + 3) & ~3;
  const int64_t ab = n.t.e2e_tab.arc_off[q];
  double *B = reinterpret_cast<double *>(lds_raw);             // [2][MS]: log alpha (forward), log beta (backward)
  double *AL = LARGE ? nullptr : B + 2 * MS;                   // [MS]: log alpha_t (resident backward)
  double *TERM = LARGE ? p.terms + ab : AL + MS;               // [arcs]: the frame's terms
  float *E = reinterpret_cast<float *>(LARGE ? B + 2 * MS : TERM + MA);  // [MP]: the frame's y per distinct pdf
  double *hist = p.hist + (int64_t)n.T * v.sb;                 // [T][n]: log alpha_t
  double *arcs = p.arcs + ab, *finals = p.finals + v.sb;
  const int start = n.t.e2e_tab.start[q];

  int pk[kArcPdfRegs];  // the first pdfs this thread owns (-1: none)
  float ynx[kArcPdfRegs];
#pragma unroll
  for (int r = 0; r < kArcPdfRegs; ++r) {
    const int k = tid + r * kArcThreads;
    pk[r] = k < v.np ? v.pdf_of[k] : -1;
    ynx[r] = pk[r] >= 0 ? load_y<El>(n, q, 0, pk[r]) : 0.f;
  }
  bool bad = false;
  // frame t's y into E; `ahead` (-1: none) is the frame the registers fetch next
  auto stage_y = [&](int t, int ahead) {
#pragma unroll
    for (int r = 0; r < kArcPdfRegs; ++r) {
      if (pk[r] < 0) continue;
      E[tid + r * kArcThreads] = ynx[r];
      bad |= !(ynx[r] - ynx[r] == 0.f);
      if (ahead >= 0) ynx[r] = load_y<El>(n, q, ahead, pk[r]);
    }
    for (int k = tid + kArcPdfRegs * kArcThreads; k < v.np; k += kArcThreads) {  // (handles of _create_e2e_any only)
      const float y = load_y<El>(n, q, t, v.pdf_of[k]);
      E[k] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward: num_e2e_kernel's, the history into the workspace ----
  for (int i = tid; i < v.n; i += kArcThreads) B[i] = i == start ? 0.0 : -INFINITY;
  int c = 0;
  for (int t = 0; t < T; ++t) {
    stage_y(t, t + 1 < T ? t + 1 : -1);
    __syncthreads();
    const double *a_cur = B + c * MS;
    double *a_nxt = B + (1 - c) * MS;
    for (int j = tid; j < v.n; j += kArcThreads) {
      hist[(int64_t)t * v.n + j] = a_cur[j];
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

  // log Z over the final states, by a fixed-order reduction
  const double *a_T = B + c * MS;
  double logz;
  bool any_bad;
  {
    double mx = -INFINITY;
    for (int i = tid; i < v.n; i += kArcThreads) mx = fmax(mx, a_T[i] + (double)v.final_lw[i]);
    mx = e2e_wave_max_d(mx);
    if (lane == 0) red_x[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3]));
    float sum = 0.f;
    if (mx > -INFINITY)
      for (int i = tid; i < v.n; i += kArcThreads) sum += __expf((float)(a_T[i] + (double)v.final_lw[i] - mx));
    sum = e2e_wave_sum(sum);
    const int wbad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      red_s[wave] = sum;
      red_bad[wave] = wbad;
    }
    __syncthreads();
    logz = mx > -INFINITY ? mx + log((double)((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]))) : -INFINITY;
    any_bad = (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3]) != 0 || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  }
  if (tid == 0) p.logprob[q] = any_bad ? (double)NAN : logz;
  if (any_bad || !(logz > -INFINITY)) {
    for (int k = tid; k < v.na; k += kArcThreads) arcs[k] = 0.0;
    for (int i = tid; i < v.n; i += kArcThreads) finals[i] = 0.0;
    return;
  }

  // ---- where the path ends, and log beta_T ----
  // (a thread reads log alpha_T of its own states before it overwrites them; the frames' first barrier orders the rest)
  for (int i = tid; i < v.n; i += kArcThreads) {
    const double fl = (double)v.final_lw[i];
    finals[i] = (double)__expf((float)((a_T[i] + fl) - logz));
    B[i] = fl;
  }
  c = 0;

  // ---- backward ----
  // (the registers hold frame T - 1's y: the forward pass's last fetch)
  if constexpr (!LARGE) {
    uint32_t rec[kArcSlots];
    float lw[kArcSlots];
    double acc[kArcSlots];
#pragma unroll
    for (int s = 0; s < kArcSlots; ++s) {
      const int k = tid + s * kArcThreads;
      rec[s] = 0;
      lw[s] = 0.f;
      acc[s] = 0.0;
      if (k < v.na) {
        const uint32_t key = v.out_key[k];
        rec[s] = (key & 0x7ffu) | ((uint32_t)arc_source(v.out_begin, v.n, k) << 11) | ((key >> 16) << 22);
        lw[s] = v.out_lw[k];
      }
    }
    int ob[kArcStateRegs], oe[kArcStateRegs];
    double anx[kArcStateRegs];
#pragma unroll
    for (int r = 0; r < kArcStateRegs; ++r) {
      const int i = tid + r * kArcThreads;
      ob[r] = i < v.n ? v.out_begin[i] : 0;
      oe[r] = i < v.n ? v.out_begin[i + 1] : 0;
      anx[r] = i < v.n ? hist[(int64_t)(T - 1) * v.n + i] : 0.0;
    }
    for (int t = T - 1; t >= 0; --t) {
      stage_y(t, t > 0 ? t - 1 : -1);
#pragma unroll
      for (int r = 0; r < kArcStateRegs; ++r) {
        const int i = tid + r * kArcThreads;
        if (r * kArcThreads >= v.n) break;
        if (i < v.n) {
          AL[i] = anx[r];
          if (t > 0) anx[r] = hist[(int64_t)(t - 1) * v.n + i];  // a frame ahead
        }
      }
      __syncthreads();
      const double *b_cur = B + c * MS;
      double *b_nxt = B + (1 - c) * MS;
#pragma unroll
      for (int s = 0; s < kArcSlots; ++s) {
        const int k = tid + s * kArcThreads;
        if (s * kArcThreads >= v.na) break;
        if (k < v.na) {
          const double x = (double)(lw[s] + E[rec[s] >> 22]) + b_cur[rec[s] & 0x7ffu];
          TERM[k] = x;
          acc[s] += (double)__expf((float)((AL[(rec[s] >> 11) & 0x7ffu] - logz) + x));  // (exp(-inf) = 0: an arc no path takes)
        }
      }
      if (t == 0) break;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kArcStateRegs; ++r) {
        const int i = tid + r * kArcThreads;
        if (r * kArcThreads >= v.n) break;
        if (i < v.n) b_nxt[i] = arc_logsum(TERM, ob[r], oe[r]);
      }
      c = 1 - c;
    }
#pragma unroll
    for (int s = 0; s < kArcSlots; ++s) {
      const int k = tid + s * kArcThreads;
      if (k < v.na) arcs[k] = acc[s];
    }
  } else {
    int32_t *SRC = p.src + ab;  // (arc k's source: written and read by the arc's owner alone)
    for (int k = tid; k < v.na; k += kArcThreads) SRC[k] = arc_source(v.out_begin, v.n, k);
    for (int t = T - 1; t >= 0; --t) {
      stage_y(t, t > 0 ? t - 1 : -1);
      __syncthreads();
      const double *b_cur = B + c * MS, *h_t = hist + (int64_t)t * v.n;
      double *b_nxt = B + (1 - c) * MS;
      for (int k0 = tid; k0 < v.na; k0 += kGroup * kArcThreads) {
        // kGroup arcs' records, then their log alpha and accumulators, before the first exponential (arcs behind the
        // sequence's last repeat it: loads in bounds, never consumed)
        uint32_t key[kGroup];
        float w[kGroup];
        double al[kGroup], old[kGroup];
        int src[kGroup];
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          const int k = min(k0 + g * kArcThreads, v.na - 1);
          key[g] = v.out_key[k];
          w[g] = v.out_lw[k];
          src[g] = SRC[k];
        }
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          const int k = min(k0 + g * kArcThreads, v.na - 1);
          al[g] = h_t[src[g]];
          old[g] = t == T - 1 ? 0.0 : arcs[k];
        }
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
          const int k = k0 + g * kArcThreads;
          if (k >= v.na) break;
          const double x = (double)(w[g] + E[key[g] >> 16]) + b_cur[key[g] & 0xffffu];
          TERM[k] = x;
          arcs[k] = old[g] + (double)__expf((float)((al[g] - logz) + x));
        }
      }
      if (t == 0) break;
      __syncthreads();  // (the terms' stores before their loads: see the head of the file)
      for (int i = tid; i < v.n; i += kArcThreads) b_nxt[i] = arc_logsum(TERM, v.out_begin[i], v.out_begin[i + 1]);
      c = 1 - c;
    }
  }
}

namespace {

template <typename El, bool LARGE>
int launch_arc(const NumArcParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumArcParams) =
      p.n.seq_frames ? num_arc_post_kernel<El, true, LARGE> : num_arc_post_kernel<El, false, LARGE>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kArcThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <bool LARGE>
int launch_arc(const NumArcParams &p, size_t lds, hipStream_t stream) {
  if (p.n.elem == TC_DTYPE_BF16) return launch_arc<__hip_bfloat16, LARGE>(p, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_arc<__half, LARGE>(p, lds, stream);
  return launch_arc<float, LARGE>(p, lds, stream);
}

}  // namespace

int launch_num_arc_post(const NumArcParams &p, bool large, hipStream_t stream) {
  if (!p.n.t.e2e || !p.arcs || !p.finals || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (!p.hist || (large && (!p.terms || !p.src))) return TC_ERR_WORKSPACE;
  const E2eDev &e = p.n.t.e2e_tab;
  if (!large && e2e_beyond_resident(e.max_states, e.max_arcs, e.max_pdfs)) return TC_ERR_UNSUPPORTED;
  count_launch(large ? kCntNumArcPostLarge : kCntNumArcPost);
  // laid out per sequence: no more than the handle's largest counts side by side (which the resident limits bound, and the
  // any-size rule for the large form)
  if (large) return launch_arc<true>(p, e2e_seq_lds_bytes(e.max_states, e.max_pdfs), stream);
  return launch_arc<false>(p, num_arc_lds_bytes(e.max_states, e.max_arcs, e.max_pdfs), stream);
}

}  // namespace tc
