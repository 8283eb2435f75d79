// Fused denominator forward-backward for TIED (chain-structured) graphs on gfx950 -- the kernel the
// headline metric times.
//
// What it computes: [K] DenominatorComputation::Forward() + Backward() (chain-denominator.cc), reached by the
// reference through src/my_lib_chain.cpp:129-131.  Same mapping as den_kernels.hip (one workgroup = one
// sequence = one CU, the per-frame working set in LDS) with the factorisation tied graphs allow: every
// non-self-loop arc entering a state g carries one pdf f(g), so exp(y) leaves the arc sums --
//   forward   F(g)  = sum_{h->g} w * alpha'_t(h)            one LDS gather + one FMA per arc
//             alpha_{t+1}(g) * asum_t = p_t(f(g)) * F(g) + p_t(s(g)) * w_s(g) * alpha'_t(g)
//   backward  B(h)  = sum_{h->g} w * Y_t(g),  Y_t(g) = beta_{t+1}(g) * p_t(f(g))
//             gamma_t from per-state quantities only (two integer LDS atomics per STATE, none per arc)
// -- and the schedules are OWNER-COMPUTES (schedule_owner.cpp): the thread that owns a state walks its arc
// list in both directions, so row sums never cross threads.
//
// Where the time went before this file existed: every frame each CU pulled its 6-byte-per-arc cell
// stream (344 KB per direction at C3) from L2, 26 GB per launch chip-wide -- the L2 -> CU path, not HBM and
// not the LDS gathers, set the pace.  A wave's stream is the same every frame, so this kernel keeps the
// first RESF (forward phase) / RESB (backward phase) chunks of every wave's stream in REGISTERS for the
// whole phase and streams only the remainder.  That needs the registers: addresses are uniform base +
// 32-bit lane offset (SGPR-pair + one VGPR instead of 64-bit per-lane pointers), the 16-bit LDS offsets of
// resident cells are unpacked on the fly (the compiler would otherwise hoist the unpacking out of the frame
// loop and spend one more register per cell), and a row end costs one scalar bit test per cell.
#include "den_tied_frames.h"

namespace tc {

namespace {

// (the frames themselves: den_tied_frames.h, shared with den_tied_mitm.hip)
// RAGGED (DenParams::seq_frames): the sequence runs its own T_s frames (launch_den_mode passes no fwd_norm then; batches
// of 8 sequences up to half the chip take den_tied_mitm.hip's RAGGED instantiation instead)
// FULL: the twin for full layouts (tied_full_layout below; den_tied_frames.h says what it leaves out)
template <int JV, int PV, bool ALPHA_LDS, bool ACCUM, bool WANT_DERIV, int RESF, int RESB, bool RAGGED = false, bool FULL = false>
__global__ __launch_bounds__(kThreads) void den_tied_kernel(const DenParams p) {
  static_assert(!(FULL && RAGGED), "ragged batches run the general form");
  TiedSeq<JV, PV, ALPHA_LDS, ACCUM, RESF, RESB, false, FULL> q(p, (int)blockIdx.x, 0, RAGGED ? ragged_frames(p.seq_frames(), (int)blockIdx.x, p.T) : 0);
  const int T = q.T;
  // ---- forward: alpha'_0, frames 1..T, total probability
  q.forward_begin();
  for (int t = 1; t <= T; ++t) q.template forward_frame<false>(t);
  q.forward_store_row(T);
  q.stamps_flush(0);
  const float tot = q.forward_total(0.0);
  if (p.fwd_norm) {  // two-CU form: the normalisers the combining pass needs (den_tied_split.hip)
    float *const fn = p.fwd_norm + (int64_t)q.s * (T + 2);
    for (int i = (int)q.tid; i <= T; i += kThreads) fn[i] = ldsf(q.aAsum + 4u * (uint32_t)i);
    if (q.tid == 0) fn[T + 1] = tot;
  }
  if (!WANT_DERIV) return;
  // ---- backward: beta'_T = 1 / tot, frames T-1..0 with gamma
  q.template backward_begin<false>(__builtin_amdgcn_rcpf(tot));
  for (int t = T - 1; t > 0; --t) q.template backward_frame<false>(t, T);
  q.template backward_frame<false>(0, T);
  q.stamps_flush(128);
}

// Resident chunks per phase for each instantiation: what the 128 registers of a 1024-thread workgroup hold
// next to the per-thread state (JV float4s of states, PV float4s of pdfs).
#ifndef TC_RESF
#define TC_RESF 4
#endif
#ifndef TC_RESB
#define TC_RESB 4
#endif
// The full-layout twin's forward phase.  The kernel's register count is set by the backward phase, which holds next to
// its resident chunks and the two stream buffers the owned states' beta and alpha' and two rows of y; the forward phase
// holds the chunks, the buffers and one row of y, so 24 registers of every thread -- two chunks -- lie idle for its
// frames.  Only the twin can take them: it compiles to 128 VGPRs without a spill, where the general form, at 128 with 4
// spilled already, would spill 15 (profiles/fwd_resident/README.md).  RESB stays: the backward phase has none left.
#ifndef TC_RESF_FULL
#define TC_RESF_FULL 6
#endif
#ifndef TC_RES_JV3
#define TC_RES_JV3 4
#endif
#ifndef TC_RES_JV4
#define TC_RES_JV4 2
#endif
constexpr int res_fwd(int jv, int pv) { return jv > 3 ? (pv == 1 ? TC_RES_JV4 : 0) : jv == 3 ? (pv == 1 ? TC_RES_JV3 : 0) : pv == 1 ? TC_RESF : 2; }
constexpr int res_bwd(int jv, int pv) { return jv > 3 ? (pv == 1 ? TC_RES_JV4 : 0) : jv == 3 ? (pv == 1 ? TC_RES_JV3 : 0) : pv == 1 ? TC_RESB : 2; }

template <int JV, int PV, bool RAGGED>
int launch_jp(const DenParams &p, int accumulate, size_t lds_bytes, hipStream_t stream) {
  constexpr int RF = res_fwd(JV, PV), RB = res_bwd(JV, PV);
  const bool want = p.deriv != nullptr;
  const bool al = p.L.alpha_in_lds;
  void (*k)(const DenParams) = nullptr;
  if (!want)
    k = den_tied_kernel<JV, PV, true, false, false, RF, RB, RAGGED>;
  else if (accumulate)
    k = al ? den_tied_kernel<JV, PV, true, true, true, RF, RB, RAGGED> : den_tied_kernel<JV, PV, false, true, true, RF, RB, RAGGED>;
  else
    k = al ? den_tied_kernel<JV, PV, true, false, true, RF, RB, RAGGED> : den_tied_kernel<JV, PV, false, false, true, RF, RB, RAGGED>;
  // The full-layout twin exists for 8 states per thread and one plane of pdfs (the C2 / C3 class); the other layout
  // classes would each add two instantiations of the largest kernel of the library.
  // It keeps TC_RESF_FULL forward chunks resident, not RF: what its forward phase leaves idle of the registers its backward
  // phase needs is two more chunks, and without the general form's spills it has the room (see TC_RESF_FULL above).
  if constexpr (JV == kJvSmall && PV == kPvSmall && !RAGGED) {
    if (tied_full_layout(p)) {
      constexpr int RFF = TC_RESF_FULL;
      k = accumulate ? den_tied_kernel<JV, PV, true, true, true, RFF, RB, false, true> : den_tied_kernel<JV, PV, true, false, true, RFF, RB, false, true>;
      count_launch(kCntTiedFullLayout);
    }
  }
  TC_HIP_CHECK(allow_dynamic_lds((const void *)k, lds_bytes));
  hipLaunchKernelGGL(k, dim3(p.S), dim3(kThreads), lds_bytes, stream, p);
  TC_HIP_CHECK(hipGetLastError());
  return TC_OK;
}

}  // namespace

static_assert(TC_RESF <= kTiedMinChunks && TC_RESB <= kTiedMinChunks, "the resident prefix must exist in every wave's stream");
static_assert(TC_RESF_FULL <= kTiedMinChunks && TC_RESF_FULL % 2 == 0, "the resident prefix must exist in every wave's stream");

// Whether a launch takes the full-layout twin: everything TiedSeq<..., FULL> takes for granted, checked here.
//   * 8 states per thread and one plane of pdfs, every float4 of both in use (8192 positions, 4096 pdfs);
//   * the roomy layout with room for the two parked per-state tables;
//   * rows of y and of the derivative that take 16-byte accesses;
//   * no cross-entropy output to zero (so its rows' alignment, x_vec, has no reader), no hub states in either schedule,
//     a uniform batch, a derivative asked for;
//   * not a diagnostic build: the phase stamps and the ablations are statements about the general form.
bool tied_full_layout(const DenParams &p) {
#if defined(TC_PHASE_STAMPS) || defined(TC_ABL_NOATOM) || defined(TC_ABL_NODERIV) || defined(TC_ABL_NOFADD) || defined(TC_ABL_NOGAM) || \
    defined(TC_ABL_NOGATHER) || defined(TC_ABL_NOHIST) || defined(TC_ABL_NOHISTLOAD) || defined(TC_ABL_NOPARK) ||                      \
    defined(TC_ABL_NOSTREAM) || defined(TC_ABL_NOWALKSTORE) || defined(TC_ABL_NOY2) || defined(TC_NO_BWD_DEFER) || defined(TC_NO_HIST_DMA)
  return false;
#else
  if (debug_flag(kDbgNoFullLayout)) return false;
  if (p.L.JV != kJvSmall || p.L.PV != kPvSmall || p.L.planewise) return false;
  if (p.L.Hs != 4 * kThreads * kJvSmall || p.L.Ps != 4 * kThreads * kPvSmall || p.P != p.L.Ps) return false;
  if (!p.L.alpha_in_lds || p.L.off_red - p.L.off_g < 2 * p.L.Hs) return false;
  if (!p.deriv || !p.y_vec || !p.d_vec || p.xent_zero) return false;
  if (p.fwd.nfix != 0 || p.bwd.nfix != 0) return false;
  return p.seq_frames() == nullptr;
#endif
}

int launch_den_tied(const DenParams &p, int accumulate, hipStream_t stream) {
  const size_t lds = (size_t)layout_lds_bytes(p.L, p.T);
  if (lds > (size_t)kLdsLimitBytes) return TC_ERR_UNSUPPORTED;
  const int JV = p.L.JV, PV = p.L.PV;
  if (p.seq_frames() && p.fwd_norm) return TC_ERR_INVALID_ARGUMENT;  // (a ragged batch has no two-pass form: the normalisers' stride is the longest sequence's; its two-workgroup form is den_tied_mitm.hip's)
#define TC_CALL(J, V) (p.seq_frames() ? launch_jp<J, V, true>(p, accumulate, lds, stream) : launch_jp<J, V, false>(p, accumulate, lds, stream))
  TC_TIED_DISPATCH(TC_CALL)
#undef TC_CALL
  return TC_ERR_UNSUPPORTED;
}

}  // namespace tc
