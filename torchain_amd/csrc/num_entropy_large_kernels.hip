// Entropy of an end-to-end supervision's path posterior and its gradient for sequences that do not fit num_entropy_kernel
// (num_entropy_kernels.hip), for gfx950.
//
// The resident kernel keeps four double vectors of two levels in LDS -- (log alpha, Abar), then (log beta, Bbar) -- which
// serves a sequence of about 5000 states.  The numerator's any-size kernel (num_e2e_large_kernels.hip) trains sequences of
// twice that: a transcript composed with the denominator graph is there.  This kernel is the same computation -- the head
// of num_entropy_kernels.hip states the quantity and the recursions -- one workgroup of 256 threads a sequence, the same
// tables (SeqView), the same ownership (thread j walks the arc lists of states j, j + 256, ...; thread k stages and later
// sums distinct pdfs k, k + 256, ...), every operand and every sum in the same order, the same failure conventions; on a
// handle that fits both it gives the resident kernel's bits (tc_debug_set("force_num_entropy_large", 1)).  What moves is
// where the MEANS live:
//   LDS       [2][MS] log alpha of two adjacent levels as doubles (the backward pass: log beta), [MP] the frame's y per
//             distinct pdf: 16 * ceil4(states) + 4 * ceil4(pdfs) bytes with the sequence's own sizes, which is the any-size
//             numerator's rule (e2e_large_fits) -- a handle tc_supervision_create_e2e_any builds is served here.
//   workspace the means, as doubles.  GRAD: the forward pass stores (log alpha_{t+1}(j), Abar_{t+1}(j)) as ONE 16-byte store
//             into the history's row t + 1, and level t + 2 gathers Abar_{t+1}(src) from that row: no second buffer.  Level T
//             has no history row: its means go to the sequence's first mean row, where the final reduction reads them.  The
//             backward pass keeps Bbar of two levels in the sequence's two mean rows, ping-pong, and reads (log alpha_t,
//             Abar_t) from the history as the resident kernel does.  !GRAD: no history; Abar of two levels ping-pongs in the
//             two mean rows.  A sequence's rows are 8 bytes a state: they stay in L2 between the frame that writes them and
//             the frame that reads them.
//             The per-arc gradient terms, one float an arc, always live in the workspace.
// A mean or a term stored by one thread is loaded by others of the SAME workgroup one barrier later, nowhere else: the
// workgroup barrier with its workgroup-scope release and acquire fences (ent_sync) orders that -- every wave drains its
// vector stores before the barrier and the waves of a workgroup share their CU's vector L1.  No device-scope fence, no
// atomic, nothing depends on blockIdx but the sequence's own data.  Two barriers a frame in each direction.
//
// The gathers Abar_t(src) / Bbar_{t+1}(dst) are dependent L2 loads inside the arc walk: begin -> key -> mean.  ArcAhead keeps
// them off the exp chain: a state's arc records and their means are loaded kAhead arcs at a time, the next group issued
// before the current one's exponentials are consumed, and the state's first group (with the next state's list bounds) before
// the current state's logarithm.  Groups change when loads are issued, never the order of a sum.  y keeps the resident
// kernel's frame-ahead register prefetch for a thread's first four pdfs.  profiles/num_entropy_large/README.md: what it costs.
#include <float.h>
#include <math.h>

#include "chain_internal.h"
#include "half_io.h"
#include "num_e2e_device.h"

namespace tc {

namespace {

constexpr int kEntLThreads = kE2eThreads;
constexpr int kEntLPdfRegs = TC_E2E_MAX_PDFS / kEntLThreads;
#ifndef TC_NUM_ENT_LARGE_AHEAD
#define TC_NUM_ENT_LARGE_AHEAD 4
#endif
constexpr int kAhead = TC_NUM_ENT_LARGE_AHEAD;  // arcs whose records and means are in flight ahead of their use

// the workgroup's barrier: release of this wave's global and LDS stores, barrier, acquire (what __syncthreads() is)
__device__ __forceinline__ void ent_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ double entl_wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename El>
__device__ __forceinline__ void entl_store(void *g, int64_t i, float v) {
  if constexpr (std::is_same<El, float>::value)
    reinterpret_cast<float *>(g)[i] = v;
  else
    reinterpret_cast<uint16_t *>(g)[i] = Elem<El>::round(v);
}

template <typename El>
__device__ __forceinline__ void entl_store_grad(const NumEntParams &p, int q, int t, int pdf, float v) {
  if (p.n.y_bct)
    entl_store<El>(p.grad, ((int64_t)q * p.n.P + pdf) * p.n.T + t, v);
  else
    reinterpret_cast<float *>(p.grad)[((int64_t)t * p.n.S + q) * p.grad_stride + pdf] = v;
}

// kAhead arcs of one state's list: the record (key, lw) and the other level's mean of the state the key names.  Arcs behind
// the list's end repeat its last arc (a load in bounds, never consumed).
struct ArcAhead {
  uint32_t k[kAhead];
  float w[kAhead];
  double m[kAhead];
  // `ms`: doubles between two states' means (2 in a history row, 1 in a mean row)
  __device__ __forceinline__ void load(int a0, int e, const uint32_t *key, const float *lw, const double *ma, int ms) {
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int a = min(a0 + i, e - 1);
      k[i] = key[a];
      w[i] = lw[a];
    }
#pragma unroll
    for (int i = 0; i < kAhead; ++i) m[i] = ma[(int64_t)(k[i] & 0xffffu) * ms];
  }
};

// One state's step of either recursion over its arc list [b, e), ent_row of num_entropy_kernels.hip operand for operand:
// `la` (LDS) the other level's log weights, `ma` (workspace, stride `ms`) its means.  TERMS (the backward pass): the arc's
// gradient term on the way.  `first`: the list's first group, loaded by the caller ahead of this call.
template <bool TERMS>
__device__ __forceinline__ void entl_row(int b, int e, const ArcAhead &first, const uint32_t *key, const float *lw, const float *E,
                                         const double *la, const double *ma, int ms, double *la_out, double *ma_out, double al,
                                         double dv, float *term) {
  double mx = -INFINITY;
  ArcAhead cur = first, nxt = first;
  for (int a0 = b; a0 < e; a0 += kAhead) {
    if (a0 + kAhead < e) {
      if (TERMS)
        nxt.load(a0 + kAhead, e, key, lw, ma, ms);
      else {  // (the forward pass's first walk takes no mean)
#pragma unroll
        for (int i = 0; i < kAhead; ++i) {
          const int a = min(a0 + kAhead + i, e - 1);
          nxt.k[i] = key[a];
          nxt.w[i] = lw[a];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      if (a0 + i >= e) break;
      const int o = (int)(cur.k[i] & 0xffffu);
      const double r = (double)(cur.w[i] + E[cur.k[i] >> 16]);
      const double x = la[o] + r;
      mx = fmax(mx, x);
      if (TERMS) {
        const float occ = __expf((float)(al + x));  // (exp(-inf) = 0: an arc no path takes)
        term[a0 + i] = occ > 0.f ? (float)((double)occ * (dv + r + cur.m[i])) : 0.f;
      }
    }
    cur = nxt;
  }
  double acc = mx, mean = 0.0;
  if (mx > -INFINITY) {
    float sum = 0.f;
    double num = 0.0, den = 0.0;
    cur = first;
    for (int a0 = b; a0 < e; a0 += kAhead) {
      if (a0 + kAhead < e) nxt.load(a0 + kAhead, e, key, lw, ma, ms);
#pragma unroll
      for (int i = 0; i < kAhead; ++i) {
        if (a0 + i >= e) break;
        const int o = (int)(cur.k[i] & 0xffffu);
        const double r = (double)(cur.w[i] + E[cur.k[i] >> 16]);
        const float sh = __expf((float)(la[o] + r - mx));
        sum += sh;
        if (sh > 0.f) {  // (a share of 0 may stand before an infinite cost)
          num += (double)sh * (cur.m[i] + r);
          den += (double)sh;
        }
      }
      cur = nxt;
    }
    acc = mx + log((double)sum);
    mean = num / den;
  }
  *la_out = acc;
  *ma_out = mean;
}

}  // namespace

template <typename El, bool RAGGED, bool GRAD>
__global__ __launch_bounds__(kEntLThreads) void num_entropy_large_kernel(const NumEntParams p) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_x[4], red_n[4], red_d[4];
  __shared__ float red_s[4];
  __shared__ int red_bad[4];

  const NumParams &n = p.n;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = RAGGED ? n.seq_frames[q] : n.T;
  const SeqView v = seq_view(n, q);  // (its hist and stage point into the pool slot: not used here)
  const int MS = (v.n + 3) & ~3;
  double *LA = reinterpret_cast<double *>(lds_raw);   // [2][MS]: log alpha (forward), log beta (backward)
  float *E = reinterpret_cast<float *>(LA + 2 * MS);  // [v.np]: the frame's y per distinct pdf
  double *ROW = p.means + (int64_t)2 * v.sb;          // [2][v.n]: the sequence's two mean rows
  float *TERM = nullptr;                              // [arcs]: the frame's gradient terms (backward)
  double *hist = nullptr;                             // [T][n][2]: (log alpha_t, Abar_t)
  if (GRAD) {
    TERM = p.terms + n.t.e2e_tab.arc_off[q];
    hist = p.hist + (int64_t)2 * n.T * v.sb;
  }
  const int start = n.t.e2e_tab.start[q];

  if (GRAD) {  // +0 everywhere; the backward pass stores over it behind the barriers of the forward pass
    if (n.y_bct) {
      const int64_t base = (int64_t)q * n.P * n.T, cnt = (int64_t)n.P * n.T;
      for (int64_t i = tid; i < cnt; i += kEntLThreads) entl_store<El>(p.grad, base + i, 0.f);
    } else {
      float *g = reinterpret_cast<float *>(p.grad);
      for (int t = 0; t < n.T; ++t) {
        float *row = g + ((int64_t)t * n.S + q) * p.grad_stride;
        for (int j = tid; j < n.P; j += kEntLThreads) row[j] = 0.f;
      }
    }
  }

  int pk[kEntLPdfRegs];  // the first pdfs this thread owns (-1: none)
  float ynx[kEntLPdfRegs];
#pragma unroll
  for (int r = 0; r < kEntLPdfRegs; ++r) {
    const int k = tid + r * kEntLThreads;
    pk[r] = k < v.np ? v.pdf_of[k] : -1;
    ynx[r] = pk[r] >= 0 ? load_y<El>(n, q, 0, pk[r]) : 0.f;
  }
  bool bad = false;
  // frame t's y into E; `ahead` (-1: none) is the frame the registers fetch next
  auto stage_y = [&](int t, int ahead) {
#pragma unroll
    for (int r = 0; r < kEntLPdfRegs; ++r) {
      if (pk[r] < 0) continue;
      E[tid + r * kEntLThreads] = ynx[r];
      bad |= !(ynx[r] - ynx[r] == 0.f);
      if (ahead >= 0) ynx[r] = load_y<El>(n, q, ahead, pk[r]);
    }
    for (int k = tid + kEntLPdfRegs * kEntLThreads; k < v.np; k += kEntLThreads) {
      const float y = load_y<El>(n, q, t, v.pdf_of[k]);
      E[k] = y;
      bad |= !(y - y == 0.f);
    }
  };

  // ---- forward ----
  // level 0's means: the history's row 0 with a gradient, mean row 0 without (and for a sequence of no frame)
  for (int i = tid; i < v.n; i += kEntLThreads) {
    const double a0 = i == start ? 0.0 : -INFINITY;
    LA[i] = a0;
    ROW[i] = 0.0;
    if (GRAD) *reinterpret_cast<double2 *>(hist + (int64_t)2 * i) = make_double2(a0, 0.0);
  }
  int c = 0;
  for (int t = 0; t < T; ++t) {
    stage_y(t, t + 1 < T ? t + 1 : -1);
    ent_sync();
    const double *a_cur = LA + c * MS;
    double *a_nxt = LA + (1 - c) * MS;
    // where level t's means lie and where level t + 1's go
    const double *m_cur = GRAD ? hist + (int64_t)2 * t * v.n + 1 : ROW + (int64_t)c * v.n;
    const int ms = GRAD ? 2 : 1;
    const bool to_hist = GRAD && t + 1 < T;
    double *h_nxt = GRAD ? hist + (int64_t)2 * (t + 1) * v.n : nullptr;  // (dereferenced while to_hist only)
    double *m_nxt = GRAD ? ROW : ROW + (int64_t)(1 - c) * v.n;
    int j = tid, b = 0, e = 0;
    ArcAhead first;
    if (j < v.n) {
      b = v.in_begin[j];
      e = v.in_begin[j + 1];
      if (e > b) first.load(b, e, v.in_key, v.in_lw, m_cur, ms);
    }
    while (j < v.n) {
      // the next state's bounds and first group under this state's walk
      const int jn = j + kEntLThreads;
      int bn = 0, en = 0;
      ArcAhead fn;
      if (jn < v.n) {
        bn = v.in_begin[jn];
        en = v.in_begin[jn + 1];
        if (en > bn) fn.load(bn, en, v.in_key, v.in_lw, m_cur, ms);
      }
      double la_j, ma_j;
      entl_row<false>(b, e, first, v.in_key, v.in_lw, E, a_cur, m_cur, ms, &la_j, &ma_j, 0.0, 0.0, nullptr);
      a_nxt[j] = la_j;
      if (to_hist)
        *reinterpret_cast<double2 *>(h_nxt + (int64_t)2 * j) = make_double2(la_j, ma_j);
      else
        m_nxt[j] = ma_j;
      j = jn;
      b = bn;
      e = en;
      first = fn;
    }
    ent_sync();
    c = 1 - c;
  }
  const double *m_T = GRAD ? ROW : ROW + (int64_t)c * v.n;  // level T's means

  // log Z and E[log W] over the final states, by fixed-order reductions
  double logz, elw;
  bool any_bad;
  {
    const double *a_T = LA + c * MS;
    double mx = -INFINITY;
    for (int i = tid; i < v.n; i += kEntLThreads) mx = fmax(mx, a_T[i] + (double)v.final_lw[i]);
    mx = e2e_wave_max_d(mx);
    if (lane == 0) red_x[wave] = mx;
    ent_sync();
    mx = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3]));
    float sum = 0.f;
    double num = 0.0, den = 0.0;
    if (mx > -INFINITY)
      for (int i = tid; i < v.n; i += kEntLThreads) {
        const double fl = (double)v.final_lw[i];
        const float sh = __expf((float)(a_T[i] + fl - mx));
        sum += sh;
        if (sh > 0.f) {
          num += (double)sh * (m_T[i] + fl);
          den += (double)sh;
        }
      }
    sum = e2e_wave_sum(sum);
    num = entl_wave_sum_d(num);
    den = entl_wave_sum_d(den);
    const int wbad = __any(bad) ? 1 : 0;
    if (lane == 0) {
      red_s[wave] = sum;
      red_n[wave] = num;
      red_d[wave] = den;
      red_bad[wave] = wbad;
    }
    ent_sync();
    logz = mx > -INFINITY ? mx + log((double)((red_s[0] + red_s[1]) + (red_s[2] + red_s[3]))) : -INFINITY;
    elw = ((red_n[0] + red_n[1]) + (red_n[2] + red_n[3])) / ((red_d[0] + red_d[1]) + (red_d[2] + red_d[3]));
    any_bad = (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3]) != 0 || !(logz <= DBL_MAX);  // (... or NaN, +inf)
  }
  const bool ok = !any_bad && logz > -INFINITY;
  if (tid == 0) {
    p.logprob[q] = any_bad ? (double)NAN : logz;
    p.entropy[q] = ok ? logz - elw : (double)NAN;
  }
  if (!GRAD || !ok) return;

  // ---- backward, with the gradient ----
  // (every thread read its m_T in front of the reduction's last barrier: mean row 0 is free)
  const double scale = p.grad_output ? p.grad_output[q] : 1.0;
  c = 0;
  for (int i = tid; i < v.n; i += kEntLThreads) {
    const double fl = (double)v.final_lw[i];
    LA[i] = fl;
    ROW[i] = fl > -INFINITY ? fl : 0.0;
  }
  // (the registers hold frame T - 1's y: the forward pass's last fetch)
  for (int t = T - 1; t >= 0; --t) {
    stage_y(t, t > 0 ? t - 1 : -1);
    ent_sync();
    const double *b_cur = LA + c * MS, *m_cur = ROW + (int64_t)c * v.n;
    double *b_nxt = LA + (1 - c) * MS, *m_nxt = ROW + (int64_t)(1 - c) * v.n;
    const double2 *h_t = reinterpret_cast<const double2 *>(hist) + (int64_t)t * v.n;
    int i = tid, b = 0, e = 0;
    ArcAhead first;
    double2 h = make_double2(0.0, 0.0);
    if (i < v.n) {
      b = v.out_begin[i];
      e = v.out_begin[i + 1];
      h = h_t[i];
      if (e > b) first.load(b, e, v.out_key, v.out_lw, m_cur, 1);
    }
    while (i < v.n) {
      const int in = i + kEntLThreads;
      int bn = 0, en = 0;
      ArcAhead fn;
      double2 hn = make_double2(0.0, 0.0);
      if (in < v.n) {
        bn = v.out_begin[in];
        en = v.out_begin[in + 1];
        hn = h_t[in];
        if (en > bn) fn.load(bn, en, v.out_key, v.out_lw, m_cur, 1);
      }
      double lb_i, mb_i;
      entl_row<true>(b, e, first, v.out_key, v.out_lw, E, b_cur, m_cur, 1, &lb_i, &mb_i, h.x - logz, h.y - elw, TERM);
      b_nxt[i] = lb_i;
      m_nxt[i] = mb_i;
      i = in;
      b = bn;
      e = en;
      first = fn;
      h = hn;
    }
    ent_sync();  // (the terms' and the means' stores before their loads: see the head of the file)
    for (int k = tid; k < v.np; k += kEntLThreads) {
      float g = 0.f;
      for (int a = v.pdf_begin[k]; a < v.pdf_begin[k + 1]; ++a) g += TERM[v.pdf_arc[a]];
      entl_store_grad<El>(p, q, t, v.pdf_of[k], (float)(-scale * (double)g));
    }
    c = 1 - c;
  }
}

namespace {

template <typename El, bool RAGGED, bool GRAD>
int launch_entl(const NumEntParams &p, size_t lds, hipStream_t stream) {
  void (*kernel)(const NumEntParams) = num_entropy_large_kernel<El, RAGGED, GRAD>;
  TC_HIP_CHECK(allow_dynamic_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(p.n.S), dim3(kEntLThreads), lds, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

template <typename El>
int launch_entl(const NumEntParams &p, size_t lds, hipStream_t stream) {
  if (p.n.seq_frames) return p.grad ? launch_entl<El, true, true>(p, lds, stream) : launch_entl<El, true, false>(p, lds, stream);
  return p.grad ? launch_entl<El, false, true>(p, lds, stream) : launch_entl<El, false, false>(p, lds, stream);
}

}  // namespace

int launch_num_entropy_large(const NumEntParams &p, hipStream_t stream) {
  if (!p.n.t.e2e || !p.entropy || !p.logprob) return TC_ERR_INVALID_ARGUMENT;
  if (!p.means || (p.grad && (!p.hist || !p.terms))) return TC_ERR_WORKSPACE;
  const E2eDev &e = p.n.t.e2e_tab;
  // laid out per sequence: no more than the handle's largest counts side by side, and no more than the rule admits
  const size_t lds = e2e_seq_lds_bytes(e.max_states, e.max_pdfs);
  count_launch(kCntNumEntropyLarge);
  if (p.n.elem == TC_DTYPE_BF16) return launch_entl<__hip_bfloat16>(p, lds, stream);
  if (p.n.elem == TC_DTYPE_F16) return launch_entl<__half>(p, lds, stream);
  return launch_entl<float>(p, lds, stream);
}

}  // namespace tc
