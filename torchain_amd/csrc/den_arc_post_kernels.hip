// Arc and entry occupations of the denominator graph, for gfx950 (tc_den_arc_posteriors): the expected number of times each
// arc of den.fst is taken and each state is entered from the start or through the leaky-HMM jump, per sequence and summed
// over the batch -- d log Z / d log w_a, d log Z / d log pi(h) and, as the leak count, d log Z / d log c.
//
// The model is the denominator's own (den_accuracy_kernels.hip): p_t(j) = exp(clamp(y_t(j), +-kOutputLimit)), the graph's
// initial probabilities pi, the leaky-HMM coefficient c, every state final.  In Kaldi's scaling, f_t(a) = w_a p_t(pdf_a) / asum_t:
//   forward :  alpha_0 = pi;   asum_t = sum_h alpha_t(h);   alpha'_t = alpha_t + c pi asum_t   (t = 0 .. T)
//              alpha_{t+1}(g) = sum_{a: h->g} alpha'_t(h) f_t(a)
//              Z = sum_h alpha'_T(h);   log P = log Z + sum_{t<T} log asum_t
//   backward:  beta'_T = 1 / Z;   s_t = sum_h pi(h) beta'_t(h);   beta_t = beta'_t + c s_t   (t = T .. 0)
//              beta'_t(h) = sum_{a: h->g} f_t(a) beta_{t+1}(g)
// so that sum_h alpha'_t(h) beta'_t(h) = sum_h alpha_t(h) beta_t(h) = 1 at every t.  The scaled alpha_t is the true one
// over prod_{u<t} asum_u and the scaled beta'_t the true one times that product over the likelihood, so every product below
// is a posterior with no scale left over (the "scale of frame 0" of alpha_0 = pi is 1):
//   occ(a)  = sum_{t<T} alpha'_t(src_a) f_t(a) beta_{t+1}(dst_a)
//   ent(h)  = pi(h) [ beta_0(h) + c sum_{t<=T} asum_t beta'_t(h) ]      (start in h, or leak into h at level t)
//   leaks   = c sum_{t<=T} asum_t s_t                                   (= sum_h ent(h) - 1)
//
// Arithmetic.  alpha', beta, asum, 1 / asum by frame and exp(y) / asum by pdf are float32 where they are stored; every sum
// over arcs or states is accumulated in double and rounded once when it is stored.  The arc factor is the float32 product
// w * (exp(y) / asum); an arc's term is the double product the beta' sum forms anyway, f * beta_{t+1}(dst), times the double
// alpha'_t(src).  The accumulators over the frames -- one per arc, one per state -- are float32, updated as
// (float)((double)acc + term): 64 accumulators a thread fit the 128 registers a thread of a 16-wave workgroup has, 64
// doubles would not.  The cost is one rounding of 2^-24 relative a frame, about sqrt(T) * 6e-8 of an occupation.  leaks and
// log P are doubles.
//
// One workgroup of 16 wavefronts owns one sequence, one launch does everything:
//   scan    : every y of the sequence's valid frames is looked at; a NaN or +-inf gives +0 rows and NaN scalars.
//   forward : frame by frame, lane = destination state walks its in-arcs in the tables' order; alpha'_t of every frame
//             goes to the workspace, 1 / asum_t and asum_t beside it.
//   backward: frame by frame from the last.  exp(y_t) / asum_t is staged by pdf once, alpha'_t comes back from the workspace
//             once, and the thread goes through its SLOTS (chain_internal.h: DenArcDev), the by-source walk laid out on the
//             host: a slot names one arc, the same arc in every frame, so its accumulator is a register (NA slots a thread,
//             the loop unrolled) and is stored once, after the last frame, at the arc's index in tc_den_graph_arcs' order.
//             Beyond kDenArcMaxTier slots the accumulators are the thread's own floats of the sequence's workspace row
//             (NA = 0): the same operations on the same values, the same bits.
// A state's beta' sum takes its arcs in the tables' order; a row of more than kDenArcLongRow arcs is walked by its whole
// wave, lanes striding over the list, and reduced with the xor butterfly.  Sums over the states go through a wave butterfly
// and then the 16 wave sums in wave order.  State h is its thread's (h % 1024) in every loop, so beta'_t(h), beta_t(h) and
// the entry accumulator of h are written by one thread.  Nothing is atomic: a sequence's bits do not depend on the call, on
// its place in the batch or on the other sequences.
// RESIDENT: the per-frame vectors (four by state, one by pdf) are in LDS; otherwise in the workspace, through the same code.
// den_arc_reduce_kernel: the totals, one thread an element, the sequences in order, in double.
#include <float.h>
#include <math.h>

#include "chain_internal.h"

namespace tc {

namespace {

constexpr int kWavesPerGroup = kDenArcThreads / 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum of a over the workgroup, in every thread: wave butterflies, then the wave sums in wave order.  Both barriers
// are the caller's too: what was stored before the call is visible after it.
__device__ __forceinline__ double block_sum(double a, double *red, int lane, int wave) {
  a = wave_sum(a);
  __syncthreads();  // (the slots' readers of the call before)
  if (lane == 0) red[wave] = a;
  __syncthreads();
  a = 0.0;
#pragma unroll
  for (int w = 0; w < kWavesPerGroup; ++w) a += red[w];
  return a;
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

// whether any y of the sequence's T valid frames is a NaN or an infinity (every thread gets the answer)
__device__ __forceinline__ bool scan_bad(const float *y, int64_t y_stride, int S, int P, int q, int T, int lane, int wave,
                                         int *slot) {
  int bad = 0;
  for (int t = wave; t < T; t += kWavesPerGroup) {
    const float *row = y + ((int64_t)t * S + q) * y_stride;
    for (int c = lane; c < P; c += 64) bad |= !finite(row[c]);
  }
  const int any = __ballot(bad != 0) != 0;
  if (lane == 0) slot[wave] = any;
  __syncthreads();
  int all = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerGroup; ++w) all |= slot[w];
  return all != 0;
}

}  // namespace

template <int NA, bool RESIDENT>
__global__ __launch_bounds__(kDenArcThreads) void den_arc_post_kernel(const DenArcParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *red = reinterpret_cast<double *>(lds_raw);  // [kWavesPerGroup]

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.seq_frames ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int H = p.H, P = p.P, S = p.S, Hs = p.Hs;
  const int rows = NA ? NA : p.t.rows;
  float *out_arcs = p.part_arcs + (int64_t)q * p.A, *out_entries = p.part_entries + (int64_t)q * H;

  // ---- scan ----
  if (scan_bad(p.y, p.y_stride, S, P, q, T, lane, wave, reinterpret_cast<int *>(red))) {
    for (int64_t a = tid; a < p.A; a += kDenArcThreads) out_arcs[a] = 0.0f;
    for (int h = tid; h < H; h += kDenArcThreads) out_entries[h] = 0.0f;
    if (tid == 0) {
      p.logprob[q] = NAN;
      if (p.leaks) p.leaks[q] = NAN;
    }
    return;
  }

  float *seq = reinterpret_cast<float *>(p.workspace) + (int64_t)q * den_arc_seq_floats(H, P, p.T, p.t.rows);
  float *hist = seq, *inv = hist + (int64_t)(p.T + 1) * Hs, *asum = inv + den_acc_round4(p.T + 1);
  float *ws_vec = asum + den_acc_round4(p.T + 1), *ws_occ = ws_vec + den_arc_frame_floats(H, P);
  float *vec = RESIDENT ? reinterpret_cast<float *>(lds_raw + kDenArcSmallLds) : ws_vec;
  float *v0 = vec, *v1 = vec + Hs, *va = vec + 2 * Hs, *ea = vec + 3 * Hs, *pe = vec + 4 * Hs;
  const float *pi = p.t.pi;
  const double c = (double)p.leaky;

  // exp(y_t) / asum_t of frame t, by pdf (the same expression in both passes)
  auto stage = [&](int t, float inv_t) {
    const float *yrow = p.y + ((int64_t)t * S + q) * p.y_stride;
    for (int j = tid; j < P; j += kDenArcThreads) pe[j] = expf(fminf(fmaxf(yrow[j], -kOutputLimit), kOutputLimit)) * inv_t;
  };

  // ---- forward: v0 = alpha_t, va = alpha'_t ----
  double sa = 0.0;
  for (int h = tid; h < H; h += kDenArcThreads) {
    v0[h] = pi[h];
    sa += (double)pi[h];
  }
  sa = block_sum(sa, red, lane, wave);
  double Z = 0.0, lp = 0.0;
  for (int t = 0; t <= T; ++t) {
    const double ca = c * sa;
    float *ra = hist + (int64_t)t * Hs;
    double za = 0.0;
    for (int h = tid; h < H; h += kDenArcThreads) {
      const float ad = (float)((double)v0[h] + (double)pi[h] * ca);
      ra[h] = ad;
      va[h] = ad;
      za += (double)ad;
    }
    if (tid == 0) asum[t] = (float)sa;
    if (t == T) {
      Z = block_sum(za, red, lane, wave);
      break;
    }
    const float inv_t = (float)(1.0 / sa);
    if (tid == 0) inv[t] = inv_t;
    lp += log(sa);
    stage(t, inv_t);
    __syncthreads();
    sa = 0.0;
    for (int base = wave * 64; base < H; base += kDenArcThreads) {  // lane = destination state
      const int g = base + lane;
      int b = 0, e = 0;
      if (g < H) {
        b = p.t.in_begin[g];
        e = p.t.in_begin[g + 1];
      }
      auto term = [&](int i) {
        const DenAccArc a = p.t.in_arcs[i];
        return (double)va[a.other] * (double)(a.w * pe[a.pdf]);
      };
      const bool long_row = e - b > kDenArcLongRow;
      double acc = 0.0;
      if (!long_row)
        for (int i = b; i < e; ++i) acc += term(i);
      unsigned long long todo = __ballot(long_row);
      while (todo) {  // (wave-uniform)
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
        double w = 0.0;
        for (int i = bb + lane; i < ee; i += 64) w += term(i);
        w = wave_sum(w);
        if (lane == l) acc = w;
      }
      if (g < H) {
        const float na = (float)acc;
        v0[g] = na;
        sa += (double)na;
      }
    }
    sa = block_sum(sa, red, lane, wave);
  }

  // ---- backward: cb = beta_{t+1}; nb receives beta'_t, then beta_t ----
  float *cb = v0, *nb = v1;
  double leak;
  {
    const float bT = (float)(1.0 / Z);
    double sb = 0.0;
    for (int h = tid; h < H; h += kDenArcThreads) sb += (double)pi[h] * (double)bT;
    sb = block_sum(sb, red, lane, wave);  // (its first barrier: the forward pass is done with v0 and va)
    const double lb = c * sb, as_T = (double)asum[T];
    leak = as_T * lb;
    const float b = (float)((double)bT + lb);
    for (int h = tid; h < H; h += kDenArcThreads) {
      cb[h] = b;
      ea[h] = (float)(as_T * (double)bT);
    }
  }
  float occ[NA ? NA : 1];
#pragma unroll
  for (int k = 0; k < (NA ? NA : 1); ++k) occ[k] = 0.0f;
  if (!NA)
    for (int k = 0; k < rows; ++k) ws_occ[(int64_t)k * kDenArcThreads + tid] = 0.0f;
  const DenArcSlot *slots = p.t.slots + tid;

  for (int t = T - 1; t >= 0; --t) {
    stage(t, inv[t]);
    const float *ra = hist + (int64_t)t * Hs;
    if (RESIDENT)
      for (int h = tid; h < H; h += kDenArcThreads) va[h] = ra[h];
    const float *al = RESIDENT ? va : ra;
    __syncthreads();  // (pe, alpha'_t and beta of frame t + 1; the first time also the forward pass's history rows)
    double sb = 0.0, row = 0.0;
    auto slot = [&](const DenArcSlot *table, int k, float &o) {
      const DenArcSlot s = table[(int64_t)k * kDenArcThreads];
      const int src = (int)(s.meta & kDenArcSrcMask);
      if (s.meta & kDenArcValid) {
        const double term = (double)(s.w * pe[s.pdf]) * (double)cb[s.dst];
        row += term;
        o = (float)((double)o + (double)al[src] * term);
      }
      if (__ballot((s.meta & kDenArcWaveEnd) != 0)) {  // (all 64 lanes or none: the schedule's)
        row = wave_sum(row);
        if (lane != (src & 63)) row = 0.0;
      }
      if (s.meta & (kDenArcRowEnd | kDenArcWaveEnd)) {
        if ((s.meta & kDenArcRowEnd) || lane == (src & 63)) {
          const float b = (float)row;
          nb[src] = b;
          sb += (double)pi[src] * (double)b;
        }
        row = 0.0;
      }
    };
    if (NA) {
      // The unrolled loop's loads depend on nothing the frame computes -- not even on the frame -- so the compiler would
      // keep every slot in registers across the frames, or request a frame's slots up front, and spill the accumulators.
      // Tying the table's address to the accumulator a group of four slots ends with leaves 64 bytes a lane in flight.
      const DenArcSlot *sp = slots;
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        slot(sp, k, occ[k]);
        if ((k & 3) == 3) asm volatile("" : "+v"(sp), "+v"(occ[k]));
      }
    } else {
      for (int k = 0; k < rows; ++k) slot(slots, k, ws_occ[(int64_t)k * kDenArcThreads + tid]);
    }
    sb = block_sum(sb, red, lane, wave);
    const double lb = c * sb, as_t = (double)asum[t];
    leak += as_t * lb;
    for (int h = tid; h < H; h += kDenArcThreads) {  // (a state's own thread: the one that stored beta'_t(h) above)
      const double bp = (double)nb[h];
      ea[h] = (float)((double)ea[h] + as_t * bp);
      nb[h] = (float)(bp + lb);
    }
    float *x = cb;
    cb = nb;
    nb = x;
  }

  // ---- flush: every arc has one slot, every state one thread ----
  for (int h = tid; h < H; h += kDenArcThreads) out_entries[h] = (float)((double)pi[h] * ((double)cb[h] + c * (double)ea[h]));
  const int32_t *ids = p.t.slot_arc + tid;
  if (NA) {
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const int id = ids[(int64_t)k * kDenArcThreads];
      if (id >= 0) out_arcs[id] = occ[k];
    }
  } else {
    for (int k = 0; k < rows; ++k) {
      const int id = ids[(int64_t)k * kDenArcThreads];
      if (id >= 0) out_arcs[id] = ws_occ[(int64_t)k * kDenArcThreads + tid];
    }
  }
  if (tid == 0) {
    p.logprob[q] = lp + log(Z);
    if (p.leaks) p.leaks[q] = leak;
  }
}

// arc_total(a) = sum_s occ_s(a), entry_total(h) = sum_s ent_s(h): one thread an element, the sequences in order
__global__ __launch_bounds__(256) void den_arc_reduce_kernel(const float *part_arcs, const float *part_entries, int S, int64_t A,
                                                             int H, double *arc_total, double *entry_total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= A + H) return;
  const bool arc = e < A;
  const float *col = arc ? part_arcs + e : part_entries + (e - A);
  const int64_t stride = arc ? A : (int64_t)H;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += (double)col[(int64_t)s * stride];
  if (arc)
    arc_total[e] = sum;
  else
    entry_total[e - A] = sum;
}

namespace {

template <int NA, bool RESIDENT>
int launch_form(const DenArcParams &p, hipStream_t stream) {
  void (*kernel)(const DenArcParams) = den_arc_post_kernel<NA, RESIDENT>;
  const size_t lds = kDenArcSmallLds + (RESIDENT ? (size_t)4 * den_arc_frame_floats(p.H, p.P) : 0);
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kDenArcThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <int NA>
int launch_tier(const DenArcParams &p, hipStream_t stream) {
  return p.resident ? launch_form<NA, true>(p, stream) : launch_form<NA, false>(p, stream);
}

}  // namespace

int launch_den_arc_post(const DenArcParams &p, hipStream_t stream) {
  if (!p.y || !p.part_arcs || !p.part_entries || !p.logprob || !p.workspace || !p.t.slots) return TC_ERR_INVALID_ARGUMENT;
  if (p.resident && !den_arc_resident(p.H, p.P)) return TC_ERR_INVALID_ARGUMENT;
  if (p.in_registers && !p.t.tier) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenArcPost);
  if (!p.in_registers) {
    count_launch(kCntDenArcPostStreamed);
    return launch_tier<0>(p, stream);
  }
  switch (p.t.tier) {  // (= p.t.rows: the table is padded to its tier)
    case 8: return launch_tier<8>(p, stream);
    case 16: return launch_tier<16>(p, stream);
    case 32: return launch_tier<32>(p, stream);
    case 64: return launch_tier<64>(p, stream);
  }
  return TC_ERR_INVALID_ARGUMENT;
}

int launch_den_arc_reduce(const float *part_arcs, const float *part_entries, int S, int64_t A, int H, double *arc_total,
                          double *entry_total, hipStream_t stream) {
  if (!part_arcs || !part_entries || !arc_total || !entry_total || S <= 0) return TC_ERR_INVALID_ARGUMENT;
  const int64_t blocks = (A + H + 255) / 256;
  hipLaunchKernelGGL(den_arc_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, part_arcs, part_entries, S, A, H,
                     arc_total, entry_total);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace tc
