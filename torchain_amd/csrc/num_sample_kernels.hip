// Alignments drawn from a supervision's own path posterior, for gfx950 (tc_supervision_sample_paths): K whole paths per
// sequence distributed as P(path | y, supervision), for regular (time-unfolded) and end-to-end (cyclic) handles.  It is
// num_best_path_kernels.hip with a draw where that one maximises and the log semiring where that one is tropical: a forward
// pass that keeps log alpha, then a traceback that finds every choice again from the stored log alpha.  No back-pointers, no
// random numbers made here: the caller gives the uniforms, so a sample is a function of its own uniforms alone.
//
// The rule (include/torchain_hip.h states it; that text is normative).  la_t(j) is the numerator's log alpha in float64,
//     pick(weights, u): the first index, in list order, whose inclusive cumulative sum exceeds u * total; when rounding
//                       leaves none, the last index of positive weight.  A zero weight is never picked.  Doubles throughout.
//     j_T = pick(exp(la_T(i) + (double)final_lw(i) - log Z) over the states i (regular: of the last level), u[T])
//     t = T - 1 .. 0: the in-arcs a of j_{t+1} in the handle's in-list order, each weighted
//                       exp(((double)(lw_a + y_t(pdf_a)) + la_t(src_a)) - la_{t+1}(j_{t+1})),
//                     the float32 sum rounded once -- the forward pass's operand; pick with u[t]: pdf_t, and j_t = src_a.
//     score = (double)final_lw(j_T) + the terms (double)(lw_a + y_t(pdf_a)) in the order t = T - 1 .. 0.
//
// One workgroup of 256 threads owns one sequence; one launch.
// Forward: the numerator's, through its own device functions -- end-to-end: num_e2e_kernel's forward half (threads own states
// and walk their in-arc lists; maximum, float32 sum of float32 exp, double log); regular: num_device.h's num_state_log_sum
// and num_total on the level-windowed kernel's operands -- so log Z has the numerator's bits.  The history goes to the
// CALLER'S workspace (end-to-end: the rows hist[t * n + j], t = 0 .. T; regular: one double per state): the supervision's
// pool slot is read for its tables alone.
// Traceback: LEVEL-SYNCHRONOUS.  best_path's traceback is one wave chasing T dependent loads; K of those chains would each
// fetch the same rows of log alpha and the same y.  Here all K samples of a sequence step back one frame together:
//   * the four waves take the samples k = wave, wave + 4, ...; lane i of a wave keeps its wave's i-th sample -- the current
//     state, la_{t+1}(j_{t+1}) and the running score -- in registers (256 samples a pass over the levels; more samples, more
//     passes), and the wave takes them in turn, each by a shuffle from its lane;
//   * a pick is wave-wide, as den_sample_kernels.hip's: the list in chunks of 64, lane = item, an inclusive double prefix
//     over the wave on top of the chunks before, the crossing lane by ballot; a list of more than 64 items in two passes,
//     the total and then the crossing, the same sums bit for bit;
//   * STAGED form: per level the workgroup stages la_t (end-to-end: the row; regular: the level's window) and the frame's y
//     (per distinct pdf; per unique entry) in LDS once, and every sample's pick gathers from there: only the in-arc records
//     and the list bounds come from L2.  The forward pass's two double vectors become the two levels' buffers, a second y
//     buffer lies beside the first.  Level t - 1's operands are requested into registers (4 doubles and 2 floats a thread;
//     what a level has beyond that is copied where it is stored) before level t's picks and stored into the other buffer
//     after them: one barrier a level;
//   * STREAMED form (a handle whose second y buffer does not fit; "force_num_sample_streamed"): the picks read la_t from
//     the workspace and y from the caller's tensor; no barrier.  The same operands in the same orders: the staged form's bits.
// No atomics, fixed orders, one vector store per output slot; nothing depends on blockIdx but the sequence's own data.
//
// Failure: no path of T arcs (log Z = -inf: logprob -inf), or a NaN / +-inf among the y the sequence reads (logprob NaN;
// found by the threads that stage y in the forward pass).  Either way -1 in every pdf and state slot and NaN in every score
// of the sequence.  The padding slots of a ragged handle get -1, and nothing at frames >= T_s is read.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kSmpThreads = kE2eThreads;    // the numerator's 256: the forward code is shared unchanged
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpBatch = 64 * kSmpWaves;   // samples a pass over the levels: one a lane
constexpr int kSmpLaRegs = 4;               // log alpha of the next level a thread requests a level ahead
constexpr int kSmpYRegs = 2;                // y of the next frame ...

// inclusive prefix sums over the 64 lanes
__device__ __forceinline__ double smp_wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// pick(weights, u) by one wave, weight(i) the non-negative double weight of item i of n (n, u and the weights are the same
// in every lane); every lane returns the index, -1 when the total is not positive (den_sample_kernels.hip's wave_pick)
template <typename W>
__device__ __forceinline__ int smp_wave_pick(int n, float u, int lane, W weight) {
  double base = 0.0, w = 0.0, cum = 0.0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    w = c0 + lane < n ? weight(c0 + lane) : 0.0;
    cum = base + smp_wave_scan(w, lane);
    base = __shfl(cum, 63, 64);
  }
  if (!(base > 0.0)) return -1;
  const double thr = (double)u * base;
  if (n <= 64) {  // (the one chunk is still in the registers)
    const unsigned long long over = __ballot(w > 0.0 && cum > thr);
    if (over) return __ffsll((long long)over) - 1;
    return 63 - __clzll((long long)__ballot(w > 0.0));
  }
  int last = -1;
  base = 0.0;
  for (int c0 = 0; c0 < n; c0 += 64) {  // the same sums again, bit for bit
    w = c0 + lane < n ? weight(c0 + lane) : 0.0;
    cum = base + smp_wave_scan(w, lane);
    base = __shfl(cum, 63, 64);
    const unsigned long long over = __ballot(w > 0.0 && cum > thr);
    if (over) return c0 + __ffsll((long long)over) - 1;
    const unsigned long long pos = __ballot(w > 0.0);
    if (pos) last = c0 + 63 - __clzll((long long)pos);
  }
  return last;
}

// -1 into the pdf slots t >= pdf_from and the state slots t >= state_from of every sample of sequence q, by the workgroup
__device__ __forceinline__ void smp_blank(const NumSampleParams &p, int q, int pdf_from, int state_from) {
  const int Tm = p.n.T, K = p.K, tid = threadIdx.x;
  const int np = Tm - pdf_from, ns = Tm + 1 - state_from;
  int32_t *pdf = p.pdf_out + (int64_t)q * K * Tm;
  for (int64_t i = tid; i < (int64_t)K * np; i += kSmpThreads) pdf[(i / np) * Tm + pdf_from + i % np] = -1;
  if (!p.state_out) return;
  int32_t *state = p.state_out + (int64_t)q * K * (Tm + 1);
  for (int64_t i = tid; i < (int64_t)K * ns; i += kSmpThreads) state[(i / ns) * (Tm + 1) + state_from + i % ns] = -1;
}

// what a failed sequence leaves
__device__ __forceinline__ void smp_failed(const NumSampleParams &p, int q) {
  smp_blank(p, q, 0, 0);
  for (int k = threadIdx.x; k < p.K; k += kSmpThreads) p.score_out[(int64_t)q * p.K + k] = (double)NAN;
}

// The traceback of sequence q's K samples, by the whole workgroup, T its frames and logz its log Z.
//   hT, flw, f0, nf : la_T and final_lw by sequence-local state; the candidates of j_T are the states f0 .. f0 + nf - 1
//   list(j, b, c)   : the in-list of state j: positions b .. b + c - 1
//   item(t, pos, sc, src) : the list item at pos: the float32 operand lw + y_t(pdf) and the source state
//   la(t, j)        : la_t(j);   pdf(pos): the item's pdf
//   fetch(t), commit(t) : the STAGED form's requests for level t's operands, and their stores into level t's buffers
template <bool STREAMED, class List, class Item, class La, class Pdf, class Fetch, class Commit>
__device__ __forceinline__ void smp_traceback(const NumSampleParams &p, int q, int T, double logz, const double *hT,
                                              const float *flw, int f0, int nf, List list, Item item, La la, Pdf pdf,
                                              Fetch fetch, Commit commit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Tm = p.n.T, K = p.K;
  for (int k0 = 0; k0 < K; k0 += kSmpBatch) {
    // this wave's samples of the pass: k0 + wave + i * kSmpWaves, i < cnt; lane i keeps the i-th
    const int left = K - k0 - wave;
    const int cnt = left <= 0 ? 0 : min(64, (left + kSmpWaves - 1) / kSmpWaves);
    auto sample_of = [&](int i) { return (int64_t)q * K + k0 + wave + i * kSmpWaves; };
    int cur = -1;
    double la_cur = 0.0, score = (double)NAN;
    for (int i = 0; i < cnt; ++i) {
      const int64_t s = sample_of(i);
      const int x = smp_wave_pick(nf, p.uniforms[s * (Tm + 1) + T], lane,
                                  [&](int c) { return exp((hT[f0 + c] + (double)flw[f0 + c]) - logz); });
      const int j = x < 0 ? -1 : f0 + x;  // (-1 is not reached: log Z is the log-sum of these)
      if (lane == i && j >= 0) {
        cur = j;
        la_cur = hT[j];
        score = (double)flw[j];
      }
      if (lane == 0 && p.state_out) p.state_out[s * (Tm + 1) + T] = j;
    }
    if (!STREAMED) {
      __syncthreads();  // (the buffers' readers of the pass before, and of the forward pass)
      fetch(T - 1);
      commit(T - 1);
      __syncthreads();
    }
    for (int t = T - 1; t >= 0; --t) {
      if (!STREAMED && t > 0) fetch(t - 1);  // a level ahead, behind the picks
      for (int i = 0; i < cnt; ++i) {
        const int j = __builtin_amdgcn_readfirstlane(__shfl(cur, i, 64));
        const int64_t s = sample_of(i);
        int src = -1, pd = -1;
        if (j >= 0) {  // (wave-uniform)
          const double lan = __shfl(la_cur, i, 64);
          int b, c;
          list(j, b, c);
          const int x = smp_wave_pick(c, p.uniforms[s * (Tm + 1) + t], lane, [&](int k) {
            float sc;
            int sr;
            item(t, b + k, sc, sr);
            return exp(((double)sc + la(t, sr)) - lan);
          });
          if (x >= 0) {  // (else not reached: la_{t+1}(j) is the log-sum of these)
            float sc;
            item(t, b + x, sc, src);
            pd = pdf(b + x);
            const double l = la(t, src);
            if (lane == i) {
              la_cur = l;
              score += (double)sc;
            }
          }
        }
        if (lane == i) {
          cur = src;
          if (src < 0) score = (double)NAN;
        }
        if (lane == 0) {
          p.pdf_out[s * Tm + t] = pd;
          if (p.state_out) p.state_out[s * (Tm + 1) + t] = src;
        }
      }
      if (!STREAMED && t > 0) {
        commit(t - 1);
        __syncthreads();
      }
    }
    if (lane < cnt) p.score_out[sample_of(lane)] = score;
  }
}

}  // namespace

// End-to-end supervisions.  El, RAGGED: as num_e2e_kernel's.  LDS, laid out with the sequence's own sizes: [2][MS] doubles,
// log alpha of two levels, and [MP] floats, the frame's y per distinct pdf -- [2][MP] in the staged form.
template <typename El, bool RAGGED, bool STREAMED>
__global__ __launch_bounds__(kSmpThreads) void num_sample_e2e_kernel(const NumSampleParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_x[4];
  __shared__ float red_s[4];
  __shared__ int red_bad[4];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? ragged_frames(n.seq_frames, q, n.T) : n.T;
  const SeqView v = seq_view(n, q);  // (its hist and stage point into the pool slot: not used here)
  const int MS = (v.n + 3) & ~3, MP = (v.np + 3) & ~3;
  double *B = reinterpret_cast<double *>(lds_raw);  // [2][MS]
  float *E = reinterpret_cast<float *>(B + 2 * MS);  // [MP], staged: [2][MP]
  double *hist = p.hist + (int64_t)(n.T + 1) * v.sb;  // [T + 1][n]
  const int start = n.t.e2e_tab.start[q];

  // y of a frame's distinct pdfs: pdf slot tid + r * 256 waits in register r from a frame ahead
  int pk[kSmpYRegs];
  float ynx[kSmpYRegs];
#pragma unroll
  for (int r = 0; r < kSmpYRegs; ++r) {
    const int k = tid + r * kSmpThreads;
    pk[r] = k < v.np ? v.pdf_of[k] : -1;
    ynx[r] = 0.f;
  }
  bool bad = false;
  auto fetch_y = [&](int t) {
#pragma unroll
    for (int r = 0; r < kSmpYRegs; ++r)
      if (pk[r] >= 0) ynx[r] = load_y<El>(n, q, t, pk[r]);
  };
  auto stage_y = [&](float *Et, int t) {
#pragma unroll
    for (int r = 0; r < kSmpYRegs; ++r) {
      if (pk[r] < 0) continue;
      Et[tid + r * kSmpThreads] = ynx[r];
      bad |= !(ynx[r] - ynx[r] == 0.f);
    }
    for (int k = tid + kSmpYRegs * kSmpThreads; k < v.np; k += kSmpThreads) {
      const float y = load_y<El>(n, q, t, v.pdf_of[k]);
      Et[k] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward: num_e2e_kernel's, the history into the workspace ----
  for (int i = tid; i < v.n; i += kSmpThreads) B[i] = i == start ? 0.0 : -INFINITY;
  int c = 0;
  fetch_y(0);
  for (int t = 0; t < T; ++t) {
    stage_y(E, t);
    if (t + 1 < T) fetch_y(t + 1);
    __syncthreads();
    const double *a_cur = B + c * MS;
    double *a_nxt = B + (1 - c) * MS;
    for (int j = tid; j < v.n; j += kSmpThreads) {
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
  const double *a_T = B + c * MS;
  for (int i = tid; i < v.n; i += kSmpThreads) hist[(int64_t)T * v.n + i] = a_T[i];

  // log Z over the final states, by the numerator's fixed-order reduction (its barriers order the history's stores before
  // the traceback's loads)
  double logz;
  bool any_bad;
  {
    double mx = -INFINITY;
    for (int i = tid; i < v.n; i += kSmpThreads) mx = fmax(mx, a_T[i] + (double)v.final_lw[i]);
    mx = e2e_wave_max_d(mx);
    if (lane == 0) red_x[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3]));
    float sum = 0.f;
    if (mx > -INFINITY)
      for (int i = tid; i < v.n; i += kSmpThreads) sum += __expf((float)(a_T[i] + (double)v.final_lw[i] - mx));
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
  if (any_bad || !(logz > -INFINITY)) return smp_failed(p, q);
  if (T < n.T) smp_blank(p, q, T, T + 1);  // a ragged handle's padding slots

  // ---- traceback ----
  double lar[kSmpLaRegs];
  auto fetch = [&](int t) {
    const double *h = hist + (int64_t)t * v.n;
#pragma unroll
    for (int r = 0; r < kSmpLaRegs; ++r) {
      const int i = tid + r * kSmpThreads;
      if (i < v.n) lar[r] = h[i];
    }
    fetch_y(t);
  };
  auto commit = [&](int t) {
    const double *h = hist + (int64_t)t * v.n;
    double *LA = B + (t & 1) * MS;
#pragma unroll
    for (int r = 0; r < kSmpLaRegs; ++r) {
      const int i = tid + r * kSmpThreads;
      if (i < v.n) LA[i] = lar[r];
    }
    for (int i = tid + kSmpLaRegs * kSmpThreads; i < v.n; i += kSmpThreads) LA[i] = h[i];
    stage_y(E + (t & 1) * MP, t);
  };
  auto y_of = [&](int t, int up) { return STREAMED ? load_y<El>(n, q, t, v.pdf_of[up]) : E[(t & 1) * MP + up]; };
  smp_traceback<STREAMED>(
      p, q, T, logz, hist + (int64_t)T * v.n, v.final_lw, 0, v.n,
      [&](int j, int &b, int &cn) {
        b = v.in_begin[j];
        cn = v.in_begin[j + 1] - b;
      },
      [&](int t, int pos, float &sc, int &src) {
        const uint32_t key = v.in_key[pos];
        sc = v.in_lw[pos] + y_of(t, (int)(key >> 16));
        src = (int)(key & 0xffffu);
      },
      [&](int t, int j) { return STREAMED ? hist[(int64_t)t * v.n + j] : B[(t & 1) * MS + j]; },
      [&](int pos) { return v.pdf_of[v.in_key[pos] >> 16]; }, fetch, commit);
}

// Regular supervisions.  El, RAGGED: as num_windowed_kernel's.  LDS, laid out by the handle's widest level (W states, U unique
// entries of a frame): [2][W] doubles, log alpha of two adjacent levels, and [U] floats, the frame's y per unique entry --
// [2][U] in the staged form.
template <typename El, bool RAGGED, bool STREAMED>
__global__ __launch_bounds__(kSmpThreads) void num_sample_regular_kernel(const NumSampleParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double tot_sh;

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, W = n.win_states, U = n.win_uniq;
  double *B = reinterpret_cast<double *>(lds_raw);   // [2][W]
  float *Y = reinterpret_cast<float *>(B + 2 * W);   // [U], staged: [2][U]

  const int T = RAGGED ? ragged_frames(n.seq_frames, q, n.T) : n.T;
  const int64_t lo = RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(n.seq_level_off[q]) : (int64_t)q * (T + 2);
  const int sb = n.t.seq_state_off[q];
  const int ab = n.t.seq_arc_off[q];
  const int ub = n.t.seq_uniq_off[q];
  const int *level = n.t.level_begin + lo;
  const int *frame_uniq = n.t.frame_uniq + (RAGGED ? lo - q : (int64_t)q * (T + 1));
  const int *in_begin = n.t.in_begin + sb + q;
  const int *in_arc = n.t.in_arc + ab;
  const int *arc_src = n.t.arc_src + ab, *arc_uniq = n.t.arc_uniq + ab;
  const float *arc_logw = n.t.arc_logw + ab;
  const float *final_logw = n.t.final_logw + sb;
  double *hist = p.hist + sb;  // log alpha of every state of the sequence

  // y of a frame's unique entries: entry u0 + tid + r * 256 waits in register r from a frame ahead
  float ynx[kSmpYRegs] = {};
  bool bad = false;
  auto fetch_y = [&](int t) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kSmpYRegs; ++r) {
      const int u = u0 + tid + r * kSmpThreads;
      if (u < u1) ynx[r] = num_load_y<El>(n, q, ub + u);
    }
  };
  auto stage_y = [&](float *Yt, int t) __attribute__((always_inline)) {
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
#pragma unroll
    for (int r = 0; r < kSmpYRegs; ++r) {
      const int u = u0 + tid + r * kSmpThreads;
      if (u < u1) {
        Yt[u - u0] = ynx[r];
        bad |= !(ynx[r] - ynx[r] == 0.f);
      }
    }
    for (int u = u0 + tid + kSmpYRegs * kSmpThreads; u < u1; u += kSmpThreads) {
      const float y = num_load_y<El>(n, q, ub + u);
      Yt[u - u0] = y;
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
    stage_y(Y, t);
    __syncthreads();
    if (t + 1 < T) fetch_y(t + 1);
    const double *cur = B + (t & 1) * W;
    double *nxt = B + ((t + 1) & 1) * W;
    auto score = [&](int a) __attribute__((always_inline)) { return Y[arc_uniq[a] - u0] + arc_logw[a]; };
    for (int st = s1 + tid; st < s2; st += kSmpThreads) {
      const double v = num_state_log_sum(in_begin[st], in_begin[st + 1],
                                         [&](int i) __attribute__((always_inline)) { return in_arc[i]; }, score,
                                         [&](int a) __attribute__((always_inline)) { return cur[arc_src[a] - s0]; });
      nxt[st - s1] = v;
      hist[st] = v;
    }
    __syncthreads();  // (also orders the history's stores before the traceback's loads)
  }

  // log Z, the numerator's num_total: one lane
  const int f0 = level[T], f1 = level[T + 1];
  const double *last = B + (T & 1) * W;
  if (tid == 0) tot_sh = num_total(f0, f1, final_logw, [&](int st) __attribute__((always_inline)) { return last[st - f0]; });
  const bool some_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  const double logz = tot_sh;
  const bool any_bad = some_bad || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  if (tid == 0) p.logprob[q] = any_bad ? (double)NAN : logz;
  if (any_bad || !(logz > -INFINITY)) return smp_failed(p, q);
  if (T < n.T) smp_blank(p, q, T, T + 1);  // a ragged handle's padding slots

  // ---- traceback ----
  double lar[kSmpLaRegs];
  auto fetch = [&](int t) __attribute__((always_inline)) {
    const int s0 = level[t], s1 = level[t + 1];
#pragma unroll
    for (int r = 0; r < kSmpLaRegs; ++r) {
      const int st = s0 + tid + r * kSmpThreads;
      if (st < s1) lar[r] = hist[st];
    }
    fetch_y(t);
  };
  auto commit = [&](int t) __attribute__((always_inline)) {
    const int s0 = level[t], s1 = level[t + 1];
    double *LA = B + (t & 1) * W;
#pragma unroll
    for (int r = 0; r < kSmpLaRegs; ++r) {
      const int st = s0 + tid + r * kSmpThreads;
      if (st < s1) LA[st - s0] = lar[r];
    }
    for (int st = s0 + tid + kSmpLaRegs * kSmpThreads; st < s1; st += kSmpThreads) LA[st - s0] = hist[st];
    stage_y(Y + (t & 1) * U, t);
  };
  smp_traceback<STREAMED>(
      p, q, T, logz, hist, final_logw, f0, f1 - f0,
      [&](int j, int &b, int &cn) __attribute__((always_inline)) {
        b = in_begin[j];
        cn = in_begin[j + 1] - b;
      },
      [&](int t, int pos, float &sc, int &src) __attribute__((always_inline)) {
        const int a = in_arc[pos];
        const int u = arc_uniq[a];
        sc = (STREAMED ? num_load_y<El>(n, q, ub + u) : Y[(t & 1) * U + u - frame_uniq[t]]) + arc_logw[a];
        src = arc_src[a];
      },
      [&](int t, int j) __attribute__((always_inline)) { return STREAMED ? hist[j] : B[(t & 1) * W + j - level[t]]; },
      [&](int pos) __attribute__((always_inline)) { return n.t.uniq_pdf[ub + arc_uniq[in_arc[pos]]]; }, fetch, commit);
}

namespace {

template <typename El, bool RAGGED, bool STREAMED>
int launch_smp(const NumSampleParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumSampleParams) =
      p.n.t.e2e ? num_sample_e2e_kernel<El, RAGGED, STREAMED> : num_sample_regular_kernel<El, RAGGED, STREAMED>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kSmpThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename El>
int launch_smp(const NumSampleParams &p, bool streamed, size_t lds, hipStream_t stream) {
  if (p.n.seq_frames) return streamed ? launch_smp<El, true, true>(p, lds, stream) : launch_smp<El, true, false>(p, lds, stream);
  return streamed ? launch_smp<El, false, true>(p, lds, stream) : launch_smp<El, false, false>(p, lds, stream);
}

}  // namespace

int launch_num_sample_paths(const NumSampleParams &p, bool streamed, hipStream_t stream) {
  if (!p.uniforms || !p.pdf_out || !p.score_out || !p.logprob || p.K <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (!p.hist) return TC_ERR_WORKSPACE;
  size_t lds;
  if (p.n.t.e2e) {
    // laid out per sequence: no more than the handle's largest counts side by side, and no more than the rule admits
    const E2eDev &e = p.n.t.e2e_tab;
    const size_t both = num_sample_lds_bytes((e.max_states + 3) & ~3, (e.max_pdfs + 3) & ~3, streamed);
    const size_t rule = (size_t)kLdsLimitBytes - 2048;
    lds = both < rule ? both : rule;
  } else {
    // (a ragged supervision: its own level offsets come with its lengths; win_*: the widest level's counts, rounded)
    if (p.n.seq_frames && !p.n.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
    if (!p.n.t.frame_uniq || !num_sample_fits(p.n.win_states, p.n.win_uniq, streamed)) return TC_ERR_UNSUPPORTED;
    lds = num_sample_lds_bytes(p.n.win_states, p.n.win_uniq, streamed);
  }
  count_launch(kCntNumSample);
  if (streamed) count_launch(kCntNumSampleStreamed);
  if (p.n.elem == TC_DTYPE_BF16) return launch_smp<__hip_bfloat16>(p, streamed, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_smp<__half>(p, streamed, lds, stream);
  return launch_smp<float>(p, streamed, lds, stream);
}

}  // namespace tc
