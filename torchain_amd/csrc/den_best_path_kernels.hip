// Best path through the denominator graph under the network's outputs, for gfx950 (tc_den_best_path): the single
// strongest path through den.fst, a phone-LM-constrained free decoding of the minibatch.
//
// Score of a path of states h_0 .. h_T joined by arcs a_1 .. a_T:
//     log pi(h_0) + sum_{t = 1 .. T} ( log w(a_t) + y_{t-1}(pdf(a_t)) )
// pi: the graph's initial probabilities, the ones the denominator uses; a state with pi == 0 starts no path.  Every state
// is final at cost 0, as in Kaldi's denominator computation.  y is taken as it is, not clamped.  The leaky-HMM
// coefficient does not enter: it smooths a sum and is not a path.
//
// Arithmetic.  log w and log pi are float64 logarithms rounded to float32 once on the host (DenBestDev).  log w + y is one
// float32 sum, the running score is float32: one add and one max per arc, score(src) + (log w + y).  So a returned score
// is within T_s * 2^-23 * M of the float64 score of the path that is returned, M the largest running |score| along that
// path, and no returned score is lower than the float64 optimum by more than the same bound.
//
// One workgroup of 16 wavefronts owns one sequence and one launch does three things:
//   scan     : every y of the sequence's valid frames, all pdfs, is looked at once; a NaN or +-inf anywhere gives the
//              sequence score NaN and -1 in every output slot, and nothing else of it runs.
//   forward  : frame by frame, lane = destination state (64 states a wave at a time) walks its in-arcs in the tables'
//              order; a state with more than kLongRow in-arcs is walked by the whole wave instead, lanes striding over the
//              list, and reduced with a butterfly (max is exact, so the order does not show).  Every state's score goes to
//              the history row hist[t] in the workspace: (T + 1) rows of Hs floats a sequence.  RESIDENT: the previous
//              frame's scores are read from LDS (two float32 vectors, double-buffered); otherwise from the history row the
//              workgroup has just written.  A compile-time switch: the resident form pays nothing for the other.
//   traceback: by the first wavefront.  The last state is the argmax of row T (the lowest state among equals); then, for
//              t = T .. 1, the lanes evaluate the in-arcs of the current state from row t - 1 and y with the forward pass's
//              own expression -- the same float operations, so the state's maximum is found again bit for bit -- and a
//              wave reduction picks the winner, the lowest in-arc position among equals.  No back-pointers are stored.
// The tables are the graph's, the orders are fixed and nothing is atomic: the path of a sequence does not depend on its
// place in the batch, on the other sequences or on the call.  Nothing at frames t >= T_s of a ragged batch is read; the
// padding slots get -1.  A sequence none of whose paths has T_s arcs (every start state dies out) gets -inf and -1s.
//
// y is gathered by pdf straight from the caller's tensor (L2): per frame a sequence reads A arc records, A scores and A
// outputs for H results, and the traceback is a chain of T_s dependent steps of a few loads each.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"

namespace tc {

namespace {

constexpr int kDenBestThreads = 1024;
constexpr int kLongRow = 128;  // in-arcs beyond which a state's list is walked by its whole wave

// the one expression of a candidate, forward and traceback alike: two float32 additions (nothing to contract)
__device__ __forceinline__ float candidate(float prev, float logw, float y) { return prev + (logw + y); }

template <typename E>
__device__ __forceinline__ float best_y(const DenBestParams &p, int q, int t, int pdf) {
  return p.y_bct ? load_elem<E>(p.y, ((int64_t)q * p.P + pdf) * p.T + t) : p.y[((int64_t)t * p.S + q) * p.y_stride + pdf];
}

// the better of two candidates (value, position): the larger value, the lower position among equals.  A NaN is never
// taken; an empty list leaves (-inf, INT_MAX).
__device__ __forceinline__ void best_take(float &bv, int &bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// ... over the 64 lanes of a wave; every lane ends with the winner (the order is total, so all agree)
__device__ __forceinline__ void wave_best(float &bv, int &bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    best_take(bv, bi, ov, oi);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// -1 in every slot of the sequence's T frames and the given score: by the threads `tid` of `n`
__device__ __forceinline__ void no_path(const DenBestParams &p, int q, int T, double score, int tid, int n) {
  int32_t *out = p.pdf_out + (int64_t)q * p.T;
  for (int t = tid; t < T; t += n) out[t] = -1;
  if (p.state_out) {
    int32_t *sout = p.state_out + (int64_t)q * (p.T + 1);
    for (int t = tid; t <= T; t += n) sout[t] = -1;
  }
  if (tid == 0) p.score_out[q] = score;
}

}  // namespace

// E: element type of y when it is the caller's (S, P, T) tensor (2-D: float32).  RAGGED: the loop bound is the sequence's
// own.  RESIDENT: see above.
template <typename E, bool RAGGED, bool RESIDENT>
__global__ __launch_bounds__(kDenBestThreads) void den_best_path_kernel(const DenBestParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  float *lds_score = reinterpret_cast<float *>(lds_raw);  // RESIDENT: [2][Hs]

  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const int H = p.H, Hs = p.Hs;
  const int32_t *in_begin = p.t.in_begin;
  const DenBestArc *arcs = p.t.arcs;
  float *hist = p.hist + (int64_t)q * (p.T + 1) * Hs;
  int32_t *out = p.pdf_out + (int64_t)q * p.T;
  int32_t *sout = p.state_out ? p.state_out + (int64_t)q * (p.T + 1) : nullptr;

  // a ragged batch's padding slots
  for (int t = T + tid; t < p.T; t += kDenBestThreads) out[t] = -1;
  if (sout)
    for (int t = T + 1 + tid; t <= p.T; t += kDenBestThreads) sout[t] = -1;

  // ---- scan: every y of the valid frames, in the order the tensor lies in memory ----
  {
    int bad = 0;
    if (p.y_bct) {
      for (int c = wave; c < p.P; c += kDenBestThreads / 64)
        for (int t = lane; t < T; t += 64) bad |= !(fabsf(best_y<E>(p, q, t, c)) <= FLT_MAX);
    } else {
      for (int t = wave; t < T; t += kDenBestThreads / 64)
        for (int c = lane; c < p.P; c += 64) bad |= !(fabsf(best_y<E>(p, q, t, c)) <= FLT_MAX);
    }
    if (__syncthreads_or(bad)) return no_path(p, q, T, (double)NAN, tid, kDenBestThreads);
  }

  // ---- forward: row t - 1 -> row t ----
  for (int h = tid; h < H; h += kDenBestThreads) {
    const float v = p.t.logpi[h];
    hist[h] = v;
    if (RESIDENT) lds_score[h] = v;
  }
  __syncthreads();
  for (int t = 1; t <= T; ++t) {
    const float *prev = RESIDENT ? lds_score + ((t - 1) & 1) * Hs : hist + (int64_t)(t - 1) * Hs;
    float *row = hist + (int64_t)t * Hs;
    float *nxt = lds_score + (t & 1) * Hs;
    for (int base = wave * 64; base < H; base += kDenBestThreads) {  // (wave-uniform: the shuffles below see all lanes)
      const int h = base + lane;
      int b = 0, e = 0;
      if (h < H) {
        b = in_begin[h];
        e = in_begin[h + 1];
      }
      const bool long_row = e - b > kLongRow;
      float v = -INFINITY;
      if (!long_row)
        for (int i = b; i < e; ++i) {
          const DenBestArc a = arcs[i];
          v = fmaxf(v, candidate(prev[a.src], a.logw, best_y<E>(p, q, t - 1, a.pdf)));
        }
      unsigned long long todo = __ballot(long_row);
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
        float w = -INFINITY;
        for (int i = bb + lane; i < ee; i += 64) {
          const DenBestArc a = arcs[i];
          w = fmaxf(w, candidate(prev[a.src], a.logw, best_y<E>(p, q, t - 1, a.pdf)));
        }
        w = wave_max(w);
        if (lane == l) v = w;
      }
      if (h < H) {
        row[h] = v;
        if (RESIDENT) nxt[h] = v;
      }
    }
    __syncthreads();  // (also orders the history's stores before the loads of the next frame and of the traceback)
  }
  if (tid >= 64) return;

  // ---- traceback: one wavefront ----
  float total = -INFINITY;
  int st = INT_MAX;
  {
    const float *last = hist + (int64_t)T * Hs;
    for (int h = lane; h < H; h += 64) best_take(total, st, last[h], h);
  }
  wave_best(total, st);
  if (!(total > -INFINITY)) return no_path(p, q, T, (double)-INFINITY, lane, 64);
  for (int t = T; t >= 1; --t) {
    st = __builtin_amdgcn_readfirstlane(st);
    if (sout && lane == 0) sout[t] = st;
    const float *prev = hist + (int64_t)(t - 1) * Hs;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = in_begin[st] + lane; i < in_begin[st + 1]; i += 64) {
      const DenBestArc a = arcs[i];
      best_take(bv, bi, candidate(prev[a.src], a.logw, best_y<E>(p, q, t - 1, a.pdf)), i);
    }
    wave_best(bv, bi);
    if (!(bv > -INFINITY)) return no_path(p, q, T, (double)-INFINITY, lane, 64);  // (not reached: the state's score is one of these)
    const DenBestArc a = arcs[bi];
    if (lane == 0) out[t - 1] = a.pdf;
    st = a.src;
  }
  if (lane == 0) {
    if (sout) sout[0] = st;
    p.score_out[q] = (double)total;
  }
}

namespace {

template <typename E, bool RAGGED, bool RESIDENT>
int launch_den_best(const DenBestParams &p, hipStream_t stream) {
  void (*kernel)(const DenBestParams) = den_best_path_kernel<E, RAGGED, RESIDENT>;
  const size_t lds = RESIDENT ? (size_t)2 * 4 * p.Hs : 0;
  if (RESIDENT) TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kDenBestThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_den_best(const DenBestParams &p, hipStream_t stream) {
  if (p.seq_frames)
    return p.resident ? launch_den_best<E, true, true>(p, stream) : launch_den_best<E, true, false>(p, stream);
  return p.resident ? launch_den_best<E, false, true>(p, stream) : launch_den_best<E, false, false>(p, stream);
}

}  // namespace

int launch_den_best_path(const DenBestParams &p, hipStream_t stream) {
  if (!p.y || !p.hist || !p.pdf_out || !p.score_out || !p.t.arcs) return TC_ERR_INVALID_ARGUMENT;
  if (p.resident && !den_best_resident(p.H)) return TC_ERR_INVALID_ARGUMENT;
  count_launch(kCntDenBestPath);
  if (!p.resident) count_launch(kCntDenBestPathStreamed);
  if (p.elem == TC_DTYPE_BF16) return launch_den_best<__hip_bfloat16>(p, stream);
  if (p.elem == TC_DTYPE_F16) return launch_den_best<__half>(p, stream);
  return launch_den_best<float>(p, stream);
}

}  // namespace tc
