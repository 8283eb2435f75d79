// Best path of a supervision under the network's outputs, for gfx950: the frame-level pdf alignment
// (tc_supervision_best_path).  Kaldi gets it from a CPU decoder, one utterance at a time; here the numerator's tables,
// its loaders and its per-state history in the supervision's pool slot are on the device already.
//
// One workgroup of four wavefronts owns one sequence, as in the two numerator files, and one launch does both halves:
//   forward  : the numerator's forward recursion in the tropical semiring -- max where the numerator log-adds, on the
//              same operand: (double)(y + logw) + score(source), the float sum rounded once, everything else double.
//              Regular supervisions follow num_windowed_kernel (two adjacent levels of scores and the frame's y per
//              unique entry in LDS; every state's score to NumDev::alpha_hist, one double per state).  End-to-end
//              supervisions follow the forward half of num_e2e_kernel (two score vectors and the frame's y per distinct
//              pdf in LDS; the rows hist[t * n + j], t = 0 .. T, to E2eDev::alpha_hist).
//   traceback: after a barrier, by the first wavefront.  The final state is the argmax over the final states of
//              score_T + final_logw; then, for t = T - 1 .. 0, the lanes evaluate the in-arcs of the current state from
//              the history and y with the forward pass's own expression -- same precision, same order of float
//              operations, so the state's maximum is found again bit for bit -- a wave reduction picks the winner (the
//              lowest in-arc position on a tie), its pdf is the frame's output and its source the next state.
// The history is shared scratch of the slot, not state: the numerator kernels that read it write it first.  A sequence
// without a path of exactly T arcs to a final state gets score -inf and -1 in all its frames; the padding frames of a
// ragged handle get -1 and nothing at frames >= T_s is read.  No atomics, fixed orders: two runs give the same output.
//
// The traceback is a chain of T dependent steps, each a few dependent loads from L2 (arc range, arcs, y and history);
// alignment is not part of the training step, so there is one form of each kernel and no resident variant.
#include <limits.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_device.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kBestThreads = 256;

// the better of two candidates (value, position): the larger value, the lower position among equals.  A NaN is never
// taken; an empty list leaves (-inf, INT_MAX).
__device__ __forceinline__ void best_take(double &bv, int &bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// ... over the 64 lanes of a wave; every lane ends with the winner (the order is total, so all agree)
__device__ __forceinline__ void wave_best(double &bv, int &bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    best_take(bv, bi, ov, oi);
  }
}

// what a sequence without a path leaves, written by the traceback's wave
__device__ __forceinline__ void no_path(const NumParams &p, int q, int T, int lane) {
  int32_t *out = p.best_pdf + (int64_t)q * p.T;
  for (int t = lane; t < T; t += 64) out[t] = -1;
  if (lane == 0) p.best_score[q] = -INFINITY;
}

}  // namespace

// Regular supervisions.  E, RAGGED: as num_windowed_kernel's.
template <typename E = float, bool RAGGED = false>
__global__ __launch_bounds__(kBestThreads) void num_best_path_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  double *score_w = reinterpret_cast<double *>(lds_raw);               // [2][win_states]
  float *ylp = reinterpret_cast<float *>(score_w + 2 * p.win_states);  // per unique (frame, pdf) of the frame: y

  const int q = blockIdx.x, tid = threadIdx.x;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T, W = p.win_states;
  const int64_t lo = RAGGED ? (int64_t)__builtin_amdgcn_readfirstlane(p.seq_level_off[q]) : (int64_t)q * (T + 2);
  const int sb = p.t.seq_state_off[q];
  const int ab = p.t.seq_arc_off[q];
  const int ub = p.t.seq_uniq_off[q];
  const int *level = p.t.level_begin + lo;
  const int *frame_uniq = p.t.frame_uniq + (RAGGED ? lo - q : (int64_t)q * (T + 1));
  const int *in_begin = p.t.in_begin + sb + q;
  const int *in_arc = p.t.in_arc + ab;
  const int *arc_src = p.t.arc_src + ab, *arc_uniq = p.t.arc_uniq + ab;
  const float *arc_logw = p.t.arc_logw + ab;
  const float *final_logw = p.t.final_logw + sb;
  double *hist = p.t.alpha_hist + sb;
  int32_t *out = p.best_pdf + (int64_t)q * p.T;

  for (int t = T + tid; t < p.T; t += kBestThreads) out[t] = -1;  // a ragged handle's padding frames

  // ---- forward: level t -> level t + 1 ----
  if (tid == 0) {
    score_w[0] = 0.0;  // level 0 is the start state alone
    hist[0] = 0.0;
  }
  for (int t = 0; t < T; ++t) {
    const int s0 = level[t], s1 = level[t + 1], s2 = level[t + 2];
    const int u0 = frame_uniq[t], u1 = frame_uniq[t + 1];
    for (int u = u0 + tid; u < u1; u += kBestThreads) ylp[u - u0] = num_load_y<E>(p, q, ub + u);
    __syncthreads();
    const double *cur = score_w + (t & 1) * W;
    double *nxt = score_w + ((t + 1) & 1) * W;
    for (int st = s1 + tid; st < s2; st += kBestThreads) {
      double v = -INFINITY;
      for (int i = in_begin[st]; i < in_begin[st + 1]; ++i) {
        const int a = in_arc[i];
        const float sc = ylp[arc_uniq[a] - u0] + arc_logw[a];
        v = fmax(v, (double)sc + cur[arc_src[a] - s0]);
      }
      nxt[st - s1] = v;
      hist[st] = v;
    }
    __syncthreads();  // (also orders the history's stores before the traceback's loads)
  }
  if (tid >= 64) return;

  // ---- traceback: one wavefront ----
  const int lane = tid;
  const int f0 = level[T], f1 = level[T + 1];
  double total = -INFINITY;
  int st = INT_MAX;
  for (int s = f0 + lane; s < f1; s += 64) best_take(total, st, hist[s] + (double)final_logw[s], s);
  wave_best(total, st);
  if (!(total > -INFINITY)) return no_path(p, q, T, lane);
  for (int t = T - 1; t >= 0; --t) {
    st = __builtin_amdgcn_readfirstlane(st);
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = in_begin[st] + lane; i < in_begin[st + 1]; i += 64) {
      const int a = in_arc[i];
      const float sc = num_load_y<E>(p, q, ub + arc_uniq[a]) + arc_logw[a];
      best_take(bv, bi, (double)sc + hist[arc_src[a]], i);
    }
    wave_best(bv, bi);
    if (!(bv > -INFINITY)) return no_path(p, q, T, lane);  // (not reached: the state's score is one of these values)
    const int a = in_arc[bi];
    if (lane == 0) out[t] = p.t.uniq_pdf[ub + arc_uniq[a]];
    st = arc_src[a];
  }
  if (lane == 0) p.best_score[q] = total;
}

// End-to-end supervisions.  El, RAGGED: as num_e2e_kernel's.
template <typename El = float, bool RAGGED = false>
__global__ __launch_bounds__(kBestThreads) void num_e2e_best_path_kernel(const NumParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];

  const int q = blockIdx.x, tid = threadIdx.x;
  const int T = RAGGED ? ragged_frames(p.seq_frames, q, p.T) : p.T;
  const SeqView v = seq_view(p, q);
  const int MS = (v.n + 3) & ~3;  // (the sequence's own layout, as num_e2e_large_kernel's: the size rule is per sequence)
  double *A = reinterpret_cast<double *>(lds_raw);   // [2][MS]: the scores, double-buffered
  float *E = reinterpret_cast<float *>(A + 2 * MS);  // [v.np]: the frame's y per distinct pdf
  const int start = p.t.e2e_tab.start[q];
  int32_t *out = p.best_pdf + (int64_t)q * p.T;

  for (int t = T + tid; t < p.T; t += kBestThreads) out[t] = -1;  // a ragged handle's padding frames
  for (int i = tid; i < v.n; i += kBestThreads) A[i] = i == start ? 0.0 : -INFINITY;

  // ---- forward: the max walk of num_e2e_kernel ----
  int c = 0;
  for (int t = 0; t < T; ++t) {
    for (int k = tid; k < v.np; k += kBestThreads) E[k] = load_y<El>(p, q, t, v.pdf_of[k]);
    __syncthreads();
    const double *a_cur = A + c * MS;
    double *a_nxt = A + (1 - c) * MS;
    for (int j = tid; j < v.n; j += kBestThreads) {
      v.hist[(int64_t)t * v.n + j] = a_cur[j];
      double mx = -INFINITY;
      for (int i = v.in_begin[j]; i < v.in_begin[j + 1]; ++i) {
        const uint32_t key = v.in_key[i];
        mx = fmax(mx, a_cur[key & 0xffffu] + (double)(v.in_lw[i] + E[key >> 16]));
      }
      a_nxt[j] = mx;
    }
    __syncthreads();
    c = 1 - c;
  }
  for (int i = tid; i < v.n; i += kBestThreads) v.hist[(int64_t)T * v.n + i] = A[c * MS + i];
  __syncthreads();  // (orders the history's stores before the traceback's loads)
  if (tid >= 64) return;

  // ---- traceback: one wavefront ----
  const int lane = tid;
  double total = -INFINITY;
  int j = INT_MAX;
  {
    const double *h = v.hist + (int64_t)T * v.n;
    for (int i = lane; i < v.n; i += 64) best_take(total, j, h[i] + (double)v.final_lw[i], i);
  }
  wave_best(total, j);
  if (!(total > -INFINITY)) return no_path(p, q, T, lane);
  for (int t = T - 1; t >= 0; --t) {
    j = __builtin_amdgcn_readfirstlane(j);
    const double *h = v.hist + (int64_t)t * v.n;
    double bv = -INFINITY;
    int bi = INT_MAX;
    for (int i = v.in_begin[j] + lane; i < v.in_begin[j + 1]; i += 64) {
      const uint32_t key = v.in_key[i];
      best_take(bv, bi, h[key & 0xffffu] + (double)(v.in_lw[i] + load_y<El>(p, q, t, v.pdf_of[key >> 16])), i);
    }
    wave_best(bv, bi);
    if (!(bv > -INFINITY)) return no_path(p, q, T, lane);  // (not reached: the state's score is one of these values)
    const uint32_t key = v.in_key[bi];
    if (lane == 0) out[t] = v.pdf_of[key >> 16];
    j = (int)(key & 0xffffu);
  }
  if (lane == 0) p.best_score[q] = total;
}

namespace {

template <typename E, bool RAGGED>
int launch_best(const NumParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumParams) = p.t.e2e ? num_e2e_best_path_kernel<E, RAGGED> : num_best_path_kernel<E, RAGGED>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.S), dim3(kBestThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename E>
int launch_best(const NumParams &p, size_t lds, hipStream_t stream) {
  return p.seq_frames ? launch_best<E, true>(p, lds, stream) : launch_best<E, false>(p, lds, stream);
}

}  // namespace

int launch_num_best_path(const NumParams &p, hipStream_t stream) {
  if (!p.best_pdf || !p.best_score) return TC_ERR_INVALID_ARGUMENT;
  size_t lds;
  if (p.t.e2e) {
    const E2eDev &e = p.t.e2e_tab;
    // the kernel's own LDS -- two score vectors and the frame's y laid out per sequence, no static LDS; its pdfs and arcs are
    // walked in loops -- which is the per-sequence rule of the create entries: every end-to-end handle passes
    lds = e2e_seq_lds_bytes(e.max_states, e.max_pdfs);
    if (!e.alpha_hist) return TC_ERR_UNSUPPORTED;
  } else {
    // (a ragged supervision: its own level offsets come with its lengths)
    if (p.seq_frames && !p.seq_level_off) return TC_ERR_INVALID_ARGUMENT;
    lds = (size_t)p.win_states * 16 + (size_t)p.win_uniq * 4;
    if (!num_windowed_fits(lds) || !p.t.alpha_hist || !p.t.frame_uniq) return TC_ERR_UNSUPPORTED;
  }
  count_launch(kCntBestPath);
  if (p.elem == TC_DTYPE_BF16) return launch_best<__hip_bfloat16>(p, lds, stream);
  if (p.elem == TC_DTYPE_F16) return launch_best<__half>(p, lds, stream);
  return launch_best<float>(p, lds, stream);
}

}  // namespace tc
