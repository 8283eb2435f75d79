// Internal declarations shared by the host code and the HIP kernels of libtorchain_hip.so.
// Public C ABI: include/torchain_hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "torchain_hip.h"

namespace tc {

// ---- fused denominator kernel geometry ---------------------------------------------------------
// One workgroup per sequence, 16 wavefronts of 64 lanes (the CU's maximum), one workgroup per CU:
// the frame recursion is serial, so everything a sequence needs per frame lives in that CU's LDS.
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// the two kernel instantiations <JV, PV>: float4s of states / pdfs owned per thread
constexpr int kJvSmall = 2048 / kThreads, kPvSmall = 1024 / kThreads, kJvLarge = 4096 / kThreads, kPvLarge = 3072 / kThreads;
constexpr int kPvMid = 2048 / kThreads;  // 4097..8192 pdfs
constexpr int kJvMid = 3072 / kThreads;  // tied graphs of 8193..12288 positions: 12 states per thread
constexpr int kMaxRowLen = 32;             // longer in/out-arc lists are split into virtual rows
constexpr int kLdsLimitBytes = 160 * 1024; // gfx950 LDS per CU / per workgroup

// One transition as the kernels stream it: probability + two 16-bit dword indices (the state to
// gather alpha'/beta from and the pdf), 8 bytes.  [K] DenominatorGraphTransition is 12 bytes.
struct ArcRec {
  float w;
  uint32_t idx;  // state | (pdf << 16)
};

// GENERAL graphs.  A "row" is the in-arc list (forward) or out-arc list (backward) of one state, at most
// kMaxRowLen long.  Rows are sorted by length and dealt 64 at a time into "slots"; lane l of a slot walks
// row l.  Every wave gets one flat, self-describing stream of 8-byte cells laid out [pair][lane][2], so a
// wave instruction loads 64 lanes x 16 contiguous bytes and the stream is prefetched with no dependent
// address computation:
//   arc cell  : {w, pdf*4 | state*4 << 16}: the two LDS byte offsets the lane gathers from, ready to
//               use (exp(y) sits at LDS offset 0, alpha'/beta at a compile-time base that the ds_read
//               immediate supplies), so address math is one AND and one shift per cell.
//   ROW cell  : {accumulator slot | state << 16 of the row that starts here, kRowFlag | dummy offsets}.
//               It commits the previous row's sum with a plain LDS store.  All 64 lanes of a wave hit
//               their ROW cells at the same stream position, so the flag test (v_readfirstlane of
//               the cell's own offset word) feeds a scalar branch.
//   padding   : arc cell with w = 0, offsets 0 (adds 0)
// A stream ends with a ROW(dummy) cell and is padded to a multiple of kStreamUnroll cells; the whole
// array ends with readable padding so the prefetch never needs a bounds check.  Every row owns its
// accumulator slot, so no LDS float atomics are needed (ds_add_f32 costs 192 cycles per
// wave-instruction on gfx950, profiles/microbench): a state whose arc list fits one row uses slot =
// state; each further chunk of a longer list gets a private slot >= Hs + 4, and the thread that owns
// the state folds those slots in before it reads the sum ("fix-up" list, sorted by owner thread).
//
// TIED graphs use owner-computes schedules instead (schedule_owner.cpp: build_owner): states are permuted so
// that the thread owning a state walks its row, 6-byte cells without ROW cells, row ends in mask words.
constexpr uint32_t kRowFlag = 1u;  // low two bits of a cell's offset word are free (offsets are multiples of 4)
// general streams: cells per loop iteration, two 8-cell chunks in ping-pong (a third buffer was measured:
// no gain, and it pushes the fused kernel past 128 VGPRs)
constexpr int kStreamUnroll = 16;
constexpr int kStreamUnrollTied = 8;  // tied streams: a wave's range is padded to whole chunks
// ... and to at least this many chunks: the tied kernel keeps a prefix of every wave's stream in registers
// (den_tied_kernel.hip), which must exist whatever the graph
constexpr int kTiedMinChunks = 6;
constexpr int kMaxIndex = 1 << 14;
// Tied graphs of 16385..28672 positions ("plane-wise" form of the owner-computes kernel, den_tied_planes.hip; kJvPlanesSplit
// below takes it to 40960): the gather
// source alone takes 4 bytes per position of the CU's 160 KB, so a thread's 20-28 states are taken one float4 ("plane")
// at a time -- walk the four rows of the plane, then its per-state pass -- and the row sums of all planes share four
// rows per wave.  Cells carry positions (16 bits), not byte offsets.
constexpr int kJvPlanes = 7;
constexpr int kMaxPlanePositions = 4096 * kJvPlanes;
// ... and of 28673..40960 positions (round 6): the gather source no longer fits LDS as a whole, so a frame is walked in TWO
// sub-passes -- the cells whose source lies in the first half of the positions (planes 0 .. ceil(planes / 2) - 1), then,
// with the second half of the source brought in from the workspace, the others; a plane's row sums of the first sub-pass
// wait in the workspace (DenParams::part_scratch) for the second, which runs the per-state pass.  ScheduleHost::halves.
constexpr int kJvPlanesSplit = 10;
constexpr int kMaxSplitPositions = 4096 * kJvPlanesSplit;

struct ScheduleHost {
  std::vector<ArcRec> cells;       // all waves' streams, [cell][lane] (final layout [pair][lane][2])
  std::vector<uint32_t> cells6;    // tied graphs: 6-byte cells, [pair][lane]{w0, w1, off0 | off1 << 16}
  std::vector<int2> wave_range;    // kWaves x {first cell, number of cells (multiple of kStreamUnroll)}
  std::vector<int32_t> fix_begin;  // kThreads + 1: range of fix-up entries owned by each thread
  std::vector<int2> fix;           // {state, extra slot}
  int32_t extra_slots = 0;         // accumulator slots beyond Hs + 4
  int64_t conflict_cost = 0, conflict_free_cost = 0, conflict_bound = 0;  // LDS cycles of the arc gathers: as placed / if conflict-free
  int64_t real_arcs = 0, padded_arcs = 0;
  int32_t rows = 0;
  // owner-computes schedules of tied graphs (schedule_owner.cpp: build_owner)
  std::vector<uint32_t> masks;        // [wave][mask_stride]: row-end bits of pairs 8 j .. 8 j + 7 and the rows ended before its two chunks (emit_owner_stream)
  int32_t mask_stride = 0;
  std::vector<int32_t> extra_first;   // per wave: index of its first secondary-row slot group
  int32_t nfix = 0;                   // number of fix-up entries (0: no barrier after the walk)
  // plane-wise form (kMaxIndex < positions <= kMaxPlanePositions): a wave's stream is `subs` sub-streams -- its secondary
  // rows, then one per plane -- each padded to whole chunks, with mask words of its own: wave_range[wave * subs + sub],
  // masks[(wave * subs + sub) * mask_stride ...]; fix_begin is [thread][plane] (+ 1)
  int32_t subs = 0;
  // 2: split gather source (kMaxPlanePositions < positions <= kMaxSplitPositions): the wave's stream is `subs` sub-streams
  // per half (wave_range[wave * halves * subs + half * subs + sub]), a cell's field is its position inside its half,
  // fix_begin is [half][thread][plane] (+ 1)
  int32_t halves = 1;
};

struct ScheduleDev {
  const ArcRec *cells;
  const int2 *wave_range;
  const int32_t *fix_begin;
  const int2 *fix;
  const uint32_t *masks = nullptr;      // owner-computes schedules only
  const int32_t *extra_first = nullptr;
  int32_t mask_stride = 0, nfix = 0;
  const void *cells_pair = nullptr;     // tied graphs of at most 8192 positions: the stream with offsets = position * 8
  int32_t subs = 0;                     // plane-wise form: sub-streams per wave and half (ScheduleHost::subs), else 0
  int32_t halves = 1;                   // ... and the number of halves of the gather source (ScheduleHost::halves)
};

// ---- graphs too large for the on-chip layout ("streamed" path, den_slab_kernel.hip) ------------------
// alpha / beta live in HBM/L2 as [slab of G sequences][state][G] matrices, G = 16 or 32 per graph (lanes run over
// sequences, one row of a list per group of G lanes of a wave).  A LIST is a set of rows (states, or pdfs) with their entries: by destination
// (forward), by source (backward beta'), and -- general graphs only -- by pdf (gamma: one group per pdf sums its
// arcs, so the derivative needs no float atomics).  Rows are taken 64 / G at a time ("bundle"), sorted by length.
constexpr int kSlabRowsPerBlock = 64;  // rows of a list per block of 256 threads: G bundles
struct SlabRow {       // 32 bytes: two 16-byte loads per lane
  int32_t row;         // state (arc lists) or pdf (by-pdf list); -1: this group of the bundle has no row
  int32_t n;           // entries of this row
  int32_t f_off, s_off;  // tied graphs: 4 G * the state's forward / special self-loop pdf (byte offset of its row), -1: none
  float ws, pi;        // tied graphs: self-loop probability; every state list: initial probability
  float K;             // tied graphs, by destination: sum over the in-arcs of w * pi(src)
  float pad;
};
// entries: W dwords per step (tied arc lists {4 G * other state, w}: W = 2; general lists {4 G * a, 4 G * b, w, pi}:
// W = 4; by destination {src, pdf, w, pi(src)}, by source {dst, pdf, w, 1}, by pdf {src, dst, w, pi(src)}), a bundle's
// steps in chunks of 16 / W: dword c of step i of row q at [chunk][16 q + W i + c], 64 / G rows per chunk.  Steps past
// a row's end: zeros.
struct SlabListDev {
  const SlabRow *rows = nullptr;   // [bundles][64 / G]
  const int2 *head = nullptr;      // [bundles] {first chunk, steps}
  const uint32_t *rec = nullptr;   // [chunks + 3][64 / G][16]
  int32_t bundles = 0;
};
struct SlabListHost {
  int W = 2, G = 16;
  std::vector<SlabRow> rows;
  std::vector<int32_t> head;       // 2 per bundle
  std::vector<uint32_t> rec;
  int32_t bundles = 0;
};

struct BigDev {
  SlabListDev in, out, pdf;
  int G = 16;            // sequences per slab
  int in_blocks = 0, out_blocks = 0;  // blocks (of G bundles) of the two state lists; hb = the larger: rows of the per-block partials
  int hb = 0;
  // tied graphs (work-graph states): the arc lists hold the non-special arcs only and exp(y) is applied
  // per state, so an arc costs ONE row gather per pass; gamma comes from per-state quantities, added by the
  // backward kernel to fixed-point accumulators
  int tied = 0;
  const int32_t *f_off = nullptr;  // tied: per state, 4 G * forward pdf (-1: none)
};

struct DenGraphDev {
  BigDev big;
  ScheduleDev fwd, bwd;
  const float *pi;  // initial probs padded to Hs
  const uint32_t *tied_fs = nullptr;  // tied graphs: per state, forward-pdf*4 | self-loop-pdf*4 << 16
  const float *tied_w = nullptr;      // tied graphs: per state, self-loop probability (0 if none)
  void *blob = nullptr;
  // Two-sequence kernel (den_tied_pair.hip) or fused kernel for batches beyond one sequence per two CUs: decided per
  // graph and device by timing both once (api.cpp: tune_den_variant).  -1 not decided yet, -2 being decided.
  int pair_choice = -1;
  float tune_ms[2] = {0.f, 0.f};  // what the decision was made on: fused, two-sequence (ms for kTuneFrames frames)
};

// The best path through the graph (tc_den_best_path, den_best_path_kernels.hip): the FST's own states and arcs -- not the
// work graph, not layout positions -- as a CSR by destination state.  in_begin[h] .. in_begin[h + 1] are the in-arcs of
// state h in the order of the graph's arc list; log w and log pi are float64 logarithms rounded to float32 (log 0 = -inf).
struct DenBestArc {
  int32_t src, pdf;
  float logw;
};
struct DenBestDev {
  const int32_t *in_begin = nullptr;  // [H + 1]
  const DenBestArc *arcs = nullptr;   // [A]
  const float *logpi = nullptr;       // [H]
  void *blob = nullptr;
};
struct DenBestParams {
  DenBestDev t;
  const float *y;      // the 2-D float32 matrix, or the (S, P, T) tensor of `elem` (y_bct)
  int64_t y_stride;
  int y_bct, elem;
  int S, T, H, P, Hs;  // T: the longest sequence's frames; Hs: H rounded up to 4, a history row's floats
  const int32_t *seq_frames;  // [S] device, null: T each
  float *hist;         // [S][T + 1][Hs]: every state's score after t frames (the workspace)
  int32_t *pdf_out;    // [S][T]
  int32_t *state_out;  // [S][T + 1], nullable
  double *score_out;   // [S]
  int resident;        // the previous frame's scores in LDS (den_best_resident), else read from the history row
};
constexpr int kDenBestSmallLds = 1024;  // what the kernel keeps in LDS beside the two score vectors, rounded up
inline int64_t den_best_row_floats(int H) { return ((int64_t)H + 3) & ~(int64_t)3; }
inline bool den_best_resident(int H) { return 2 * 4 * den_best_row_floats(H) + kDenBestSmallLds <= (int64_t)160 * 1024; }
inline int64_t den_best_workspace_bytes(int H, int S, int T) {
  return (((int64_t)S * (T + 1) * den_best_row_floats(H) * 4) + 255) & ~(int64_t)255;
}

// The expected frame accuracy over the graph and its gradient (tc_den_expected_accuracy*, den_accuracy_kernels.hip): the
// FST's own states and arcs again, as three CSRs of the same A arcs -- by destination state (forward pass), by source
// state (backward pass) and by pdf (gradient) -- each in the order of the graph's arc list within a row.  `other` is the
// arc's source state in `in`, its destination in `out`; `pdf_arcs` carries both.  w is the handle's float32 probability.
struct DenAccArc {
  int32_t other, pdf;
  float w;
};
struct DenAccPdfArc {
  int32_t src, dst;
  float w;
};
struct DenAccDev {
  const int32_t *in_begin = nullptr, *out_begin = nullptr;  // [H + 1]
  const int32_t *pdf_begin = nullptr;                       // [P + 1]
  const DenAccArc *in_arcs = nullptr, *out_arcs = nullptr;  // [A]
  const DenAccPdfArc *pdf_arcs = nullptr;                   // [A]
  const float *pi = nullptr;                                // [H]
  void *blob = nullptr;
};
// tc_den_expected_accuracy's row kernel: m_t = sum_j gamma_t(j) a_t(j), E_s = sum_t m_t, and the scan of y
struct DenAccRowParams {
  const float *y, *gamma;
  int64_t y_stride, gamma_stride;
  int S, T, P;
  const int32_t *seq_frames;
  // The hard form: ref [S][T], pdf_class [P] nullable.  The dense form (tc_den_expected_accuracy_dense; the launchers are told
  // which): a_t(j) from row t*S + s of the float32 matrix `accuracy` (T*S, P), rows acc_stride floats apart.  The two pairs
  // share their 16 bytes, so the struct is byte for byte the one the hard form's kernels have always read.
  union {
    const int32_t *ref;
    const float *accuracy;
  };
  union {
    const int32_t *pdf_class;
    int64_t acc_stride;
  };
  float *frame_acc;  // [S][T]
  double *acc;       // [S]
};
struct DenAccGradParams {
  DenAccDev t;
  const float *y;
  int64_t y_stride;
  int S, T, H, P, Hs, Ps;  // T: the longest sequence's frames; Hs, Ps: H, P rounded up to 4
  float leaky;
  const int32_t *seq_frames;  // [S] nullable
  union {                     // as in DenAccRowParams
    const int32_t *ref;       // [S][T]
    const float *accuracy;    // (T*S, P)
  };
  union {
    const int32_t *pdf_class;  // [P] nullable
    int64_t acc_stride;
  };
  const float *frame_acc;                       // [S][T]: the centring constants m_t
  const float *seq_scale;                       // [S] nullable: 1
  float *grad;
  int64_t grad_stride;
  char *workspace;  // den_acc_grad_workspace_bytes: per sequence [alpha' | A' | 1 / asum | streamed vectors]
  int resident;     // the per-frame vectors in LDS (den_acc_resident), else in the workspace
};
__host__ __device__ inline int64_t den_acc_round4(int n) { return ((int64_t)n + 3) & ~(int64_t)3; }
// floats of the per-frame vectors: two pairs of state vectors (forward: alpha, A and alpha', A'; backward: beta, B of the
// two frames) and the frame's exp(y) / asum and centred accuracies by pdf
__host__ __device__ inline int64_t den_acc_frame_floats(int H, int P) { return 4 * den_acc_round4(H) + 2 * den_acc_round4(P); }
constexpr int kDenAccSmallLds = 1024;  // the block reductions' slots, rounded up
inline bool den_acc_resident(int H, int P) { return 4 * den_acc_frame_floats(H, P) + kDenAccSmallLds <= (int64_t)160 * 1024; }
// per sequence, in floats: alpha'_0..T, A'_0..T, 1 / asum_0..T, and room for the per-frame vectors of the streamed form
__host__ __device__ inline int64_t den_acc_seq_floats(int H, int P, int T) {
  return 2 * (int64_t)(T + 1) * den_acc_round4(H) + den_acc_round4(T + 1) + den_acc_frame_floats(H, P);
}
inline int64_t den_acc_grad_workspace_bytes(int H, int P, int S, int T) {
  return (((int64_t)S * den_acc_seq_floats(H, P, T) * 4) + 255) & ~(int64_t)255;
}

// Paths drawn from the graph's path posterior (tc_den_sample_paths, den_sample_kernels.hip): the by-destination CSR of
// DenAccDev (den_acc_tables) and nothing else of the graph.
struct DenSampleParams {
  DenAccDev t;
  const float *y;
  int64_t y_stride;
  int S, T, H, P, Hs, K;  // T: the longest sequence's frames; Hs: H rounded up to 4; K: samples a sequence
  float leaky;
  const int32_t *seq_frames;  // [S] nullable
  const float *uniforms;      // [S][K][T + 1][3]: leak decision, pre-leak state, arc (row T: the last state)
  int32_t *pdf_out;           // [S][K][T]
  int32_t *state_out;         // [S][K][T + 1][2]: pre, post; nullable
  char *workspace;            // den_sample_workspace_bytes: per sequence [alpha_0..T | asum_0..T]
  int resident;               // alpha' of the frame being read in LDS (den_sample_resident), else formed from the workspace
};
constexpr int kDenSampleSmallLds = 1024;  // the block reductions' slots, rounded up
inline bool den_sample_resident(int H) { return 4 * den_acc_round4(H) + kDenSampleSmallLds <= (int64_t)160 * 1024; }
__host__ __device__ inline int64_t den_sample_seq_floats(int H, int T) {
  return (int64_t)(T + 1) * den_acc_round4(H) + den_acc_round4(T + 1);
}
inline int64_t den_sample_workspace_bytes(int H, int S, int T) {
  return (((int64_t)S * den_sample_seq_floats(H, T) * 4) + 255) & ~(int64_t)255;
}

// Token sequences and edit distances of frame-level pdf paths (tc_paths_edit_distance, path_edit_kernels.hip)
struct PathEditParams {
  const int32_t *pdf;           // [paths][T]
  const int32_t *seq_frames;    // [paths / K] nullable
  const int32_t *token_of_pdf;  // [P]; negative: the pdf emits nothing
  const uint8_t *start_of_pdf;  // [P] nullable: null selects collapse mode
  const int32_t *ref;           // [paths / K][max_ref]; nullable when max_ref == 0
  const int32_t *ref_len;       // [paths / K]; nullable when max_ref == 0
  int32_t *dist, *len;          // [paths]
  int32_t *tokens;              // [paths][T]: the caller's, or the workspace
  int fill;                     // tokens is the caller's: -1 behind the hypothesis
  int64_t paths;                // S * K
  int K, T, P, max_ref;
};
constexpr int kPathEditWaves = 4;       // independent wavefronts a workgroup
constexpr int kPathEditMaxRef = 4096;   // a wave's previous row and reference in LDS: 4 * 2 * 4096 * 4 bytes a workgroup
inline size_t path_edit_lds_bytes(int max_ref) { return (size_t)kPathEditWaves * 2 * ((max_ref + 63) & ~63) * 4; }
inline int64_t path_edit_workspace_bytes(int S, int K, int T) { return (((int64_t)S * K * T * 4) + 255) & ~(int64_t)255; }

// The gradient of functions.sampled_risk_surrogate (tc_sampled_risk_grad, path_edit_kernels.hip); strides in elements
struct SampledRiskGradParams {
  const int32_t *pdf;         // [S][K][T]
  const int32_t *seq_frames;  // [S] nullable
  const double *weight;       // [S][K]
  const double *grad_out;     // [S]
  const void *input;
  void *grad;
  int64_t in_s, in_c, in_t, g_s, g_c, g_t;
  int S, K, T, C;
};
constexpr int kSampledRiskMaxSamples = 1024;  // a thread compares its frame's K pdfs pairwise

// LDS layout of the fused kernel, in floats: [P | A | ACC | GAMMA | ALPHA? | red | asum].  exp(y)
// (P) starts at offset 0 and its region has the compile-time size PV * 4096 of the kernel
// instantiation, so the gather source A (alpha' forward, beta backward) has a compile-time base.
struct DenLayout {
  int Hs, Ps;           // H, P rounded up to a multiple of 4
  int off_a, off_acc, off_g, off_al, off_red, off_asum, total_floats;
  bool alpha_in_lds;
  int off_p2;           // tied graphs, backward: second exp(y) buffer (frame t-1 while frame t is in use)
  int JV, PV;           // template instantiation: float4s of states / pdfs owned per thread
  int acc_floats;       // size of the accumulator region: Hs + 4 + extra slots, rounded to 4
  bool planewise = false;  // den_tied_planes.hip: [P | A | 4 rows per wave + 4 + extra slots | GAMMA | red | asum]
  // the frame sums asum_0..T live in the workspace (DenParams::asum_g), not behind off_asum: utterances too long for the
  // LDS the graph leaves (plane-wise kernel, general owner-computes kernel: the kernels they replaced ran any T)
  bool asum_global = false;
  // plane-wise form: planes of the gather source that are in LDS at a time -- JV, or ceil(JV / 2) for graphs beyond
  // kMaxPlanePositions (the gather region is 4096 * src_planes floats)
  int src_planes = 0;
};

struct DenParams {
  ScheduleDev fwd, bwd;
  const float *pi;
  const float *y;
  int64_t y_stride;
  float *deriv;
  int64_t deriv_stride;
  float *alpha_hist;    // [(T+1)][S][Hs]
  float *asum_g = nullptr;  // [S][asum_stride(T)]: the frame sums when the layout says asum_global
  // split gather source (DenLayout::src_planes < JV): the second half of the running frame's gather source
  // [S][4096 * (JV - src_planes)] and the first sub-pass's row sums [S][Hs]
  float *src_scratch = nullptr, *part_scratch = nullptr;
  double *seq_logprob;  // [S]
  double *seq_y2;       // [S] sum of y^2 (for the l2 term)
  float *seq_ab;        // [S] sum_h alpha'_0 beta'_0
  float *seq_gsum;      // [S] sum_pdf gamma_0
  int S, T, H, P;
  float leaky, deriv_weight, l2_scale;
  int y_vec, d_vec;     // rows 16-byte aligned -> float4 path
  uint32_t seq_frames_lo = 0;  // (seq_frames() below)
  // The cross-entropy output's derivative is zero outside the numerator's posteriors: kernels that write every
  // derivative row anyway (den_tied_frames.h) also write its zero rows, so that the objective call needs no memset of
  // the whole matrix in front of them (629 MB at C3: 0.13 ms).  Null: the caller has zeroed it.
  float *xent_zero = nullptr;
  int64_t xent_stride = 0;
  int x_vec = 0;
  DenLayout L;
  const uint32_t *tied_fs;  // non-null selects the tied-graph kernel (see tc_den_graph below)
  const float *tied_w;
  int gen_owner = 0;        // general graph on owner-computes schedules: den_general_owner.hip
  uint32_t seq_frames_hi = 0;
  BigDev big;           // streamed path only
  float *big_expy;      // [slab][P][16]  exp(y_t) of the current frame, transposed; or [T][slab][P][16], every frame (big_exp_stride)
  int64_t big_exp_stride = 0;  // floats between consecutive frames of big_expy (0: one frame at a time)
  float *big_beta;      // [2][slab][H][16]
  float *big_y;         // [slab][H][16]  tied graphs: Y = beta_{t+1} * p_t(f), the backward gather source
  uint32_t *big_gam = nullptr;  // [slab][P][G]  tied graphs: the frame's gamma, unsigned fixed point (den_device.h: kGammaScale)
  float *big_small;     // per-sequence sums and per-block partials (den_slab_kernel.hip: BigSmall)
  int big_Sp;           // sequences rounded up to a multiple of the slab width (big.G)
  float big_sum_pi;     // sum of the initial probabilities
  long long *stamps;    // diagnostic builds only (-DTC_PHASE_STAMPS): per-phase cycle totals, else unused
  // Two-CU form for small batches (den_tied_split.hip): the forward recursion writes its per-frame sums, the
  // backward recursion -- which does not need alpha -- runs at the same time on another CU with normalisers of
  // its own, and a third pass forms gamma from the two histories.  Null on the fused path.
  float *beta_hist = nullptr;   // [(T+1)][S][Hs]  B_t (row 0: B'_0), see den_tied_split.hip
  float *fwd_norm = nullptr;    // [S][T+2]        asum_0 .. asum_T, tot
  float *bwd_norm = nullptr;    // [S][T+1]        n_0 .. n_{T-1}
  // Two-sequence form (den_tied_pair.hip): normalisers of both roles [2][S][pair_norm_stride(T)], ticket + flags
  float *pair_norm = nullptr;
  uint32_t *pair_sync = nullptr;
  long long *pair_stamps = nullptr;  // diagnostic builds (-DTC_PAIR_STAMPS): [role][wave][T + 2][8] raw cycle stamps of pair 0
  int pair_extra_slots = 0;     // secondary-row slots of the graph's schedules (LDS layout of the pair kernel)
  int pair_choice = 0;        // the graph's tuned choice (DenGraphDev::pair_choice > 0)
  uint32_t *mitm_sync = nullptr;  // den_tied_mitm.hip: ticket + hand-over words (workspace of batches the two-CU forms may take)
  // Ragged minibatch (tc_den_forward_backward_ragged, a ragged end-to-end supervision): [S] frames of each sequence, device
  // memory.  T above stays the longest (row count, history, frame sums, LDS layout); the one-workgroup-per-sequence kernels'
  // RAGGED instantiations read their loop bound here.  Null: every sequence has T frames.  The pointer travels as two
  // 32-bit halves in what were the structure's two padding words: a new 8-byte member would move whatever follows the
  // structure among a kernel's arguments (den_tied_planes_mitm_kernel has a second one), and the uniform instantiations
  // keep their instruction streams to the byte (profiles/ragged/kernel_isa.txt).
  __host__ __device__ const int32_t *seq_frames() const {
    return reinterpret_cast<const int32_t *>(((uint64_t)seq_frames_hi << 32) | seq_frames_lo);
  }
  void set_seq_frames(const int32_t *f) {
    seq_frames_lo = (uint32_t)(uintptr_t)f;
    seq_frames_hi = (uint32_t)((uint64_t)(uintptr_t)f >> 32);
  }
};

// a ragged batch's loop bound of sequence s, held to 1 .. T: tc_den_forward_backward_ragged's lengths are device memory that
// no host code has seen, and a bound outside that range would address rows outside the caller's tensors
// (readfirstlane: DenParams rebuilds the pointer from two integers, so the compiler takes the load for a per-lane one; the
// bound must be a scalar or every frame loop's control becomes vector code)
__device__ __forceinline__ int ragged_frames(const int32_t *seq_frames, int s, int T) {
  const int f = __builtin_amdgcn_readfirstlane(seq_frames[s]);
  return f < 1 ? 1 : (f > T ? T : f);
}

}  // namespace tc

struct tc_den_graph {
  int32_t H = 0, P = 0;
  int64_t A = 0;
  std::vector<int32_t> arc_src, arc_dst, arc_pdf;
  std::vector<float> arc_prob;
  std::vector<float> initial_probs;
  tc::ScheduleHost fwd, bwd;
  // "Tied" graph: every non-self-loop arc entering a state carries the same pdf and a state has at most
  // one self-loop (chain topology after Kaldi's self-loop reordering: forward-pdf on entry, self-loop
  // pdf on the loop).  Then exp(y) factors out of the arc sums: the schedules hold only the
  // non-self-loop arcs, the forward walk gathers alpha' alone, the backward walk gathers
  // Y(g) = beta(g) * p(f(g)) alone, and the self-loops are applied per state by the owning thread.
  bool tied = false;
  // GENERAL graph on the owner-computes schedules (den_general_owner.hip, round 5): states addressed by layout position as
  // for tied graphs, 8-byte cells with the arc's pdf, no per-state tables
  bool gen_owner = false;
  std::vector<uint32_t> tied_fs;      // position order once build_owner has run
  std::vector<float> tied_w;
  std::vector<uint32_t> tied_fs_state;  // ... and in work-state order, as detect_tied left them (build_owner starts from these)
  std::vector<float> tied_w_state;
  // The graph the tied schedules are built from: the FST itself, or -- when a few states are entered
  // through arcs of more than one pdf -- its "tied-ified" version in which such a state is split into one
  // copy per entering pdf (schedule_owner.cpp: make_work_graph).  copy_first[h] .. copy_first[h+1] are the work
  // states of FST state h; work_H == H and copy_first[h] == h when nothing was split.
  int32_t work_H = 0;
  std::vector<int32_t> work_src, work_dst, work_pdf, copy_first;
  std::vector<float> work_prob, work_pi;
  std::vector<int32_t> pos;           // tied graphs: WORK state -> LDS position (see build_owner)
  std::vector<float> pi_pos;          // initial probs in position order
  tc::DenLayout layout;
  bool layout_ok = false;
  // streamed path: chosen when neither on-chip layout fits (or TC_FORCE_BIG is set)
  bool big = false;
  tc::SlabListHost big_in, big_out, big_pdf;
  int big_hb = 0;  // blocks of the longer state list (tc::BigDev::hb)
  int big_G = 16;  // sequences per slab: 32 when a slab's slice of the state matrix fits an XCD's L2 (den_graph.cpp)
  std::vector<int32_t> big_f_off;
  std::vector<int32_t> tied_f, tied_s;  // per work state: forward / special self-loop pdf, -1 if none
  float big_sum_pi = 0.f;
  std::mutex mu;
  std::map<int, tc::DenGraphDev> dev;
  std::map<int, int> preset_variant;  // device -> kernel choice fixed by the caller (tc_den_graph_set_variant)
  // tc_den_best_path's tables (den_best_path_kernels.hip), in a blob of their own per device: made on that call's first
  // use (den_best_tables, under `mu`), so `dev` and what the training step reads are what they are without it
  std::map<int, tc::DenBestDev> best_dev;
  // ... and tc_den_expected_accuracy_grad's (den_accuracy_kernels.hip, den_acc_tables), kept the same way
  std::map<int, tc::DenAccDev> acc_dev;
};

// ---- numerator -----------------------------------------------------------------------------------
namespace tc {

// Per-sequence acceptors flattened into arrays.  Local state 0 of a sequence is its (possibly
// virtual) start state; states are in time order; arcs are sorted by source state.
struct NumTables {
  std::vector<int32_t> seq_state_off, seq_arc_off, seq_uniq_off;  // S + 1 each
  std::vector<int32_t> level_begin;   // [S][T + 2] local state index where each time level begins
  std::vector<int32_t> out_begin;     // per state (+1 per sequence): arc range, local arc ids
  std::vector<int32_t> in_begin;      // per state (+1 per sequence): range into in_arc
  std::vector<int32_t> in_arc;        // per arc: local arc id, grouped by destination state
  std::vector<int32_t> arc_src, arc_dst, arc_uniq;  // local ids
  std::vector<float> arc_logw;        // -arc.weight
  std::vector<float> final_logw;      // per state: -final weight, -inf when not final
  std::vector<int32_t> uniq_t, uniq_pdf;  // per unique (frame, pdf) of a sequence
  std::vector<int32_t> uniq_begin;    // per uniq (+1 per sequence): range into uniq_arc
  std::vector<int32_t> uniq_arc;      // local arc ids in increasing order
  int32_t max_states = 0, max_arcs = 0, max_uniq = 0;
  // what the level-windowed kernel (num_windowed_kernels.hip) needs besides: where each frame's unique entries begin,
  // and the widest level / the most arcs leaving one level / the most unique entries of one frame over all sequences
  std::vector<int32_t> frame_uniq;    // [S][T + 1] sequence-local unique id where each frame's entries begin
  int32_t max_level_states = 0, max_level_arcs = 0, max_frame_uniq = 0;
  // S + 1 prefix sums of T_s + 2: where sequence s's entries of level_begin start (its frame_uniq entries start at
  // seq_level_off[s] - s).  q * (T + 2) for a uniform handle, whose kernels compute that themselves; a ragged handle
  // (tc_supervision_create_ragged) uploads it.
  std::vector<int32_t> seq_level_off;
};

// LDS of the two regular numerator kernels (launch_num, tc_supervision_stats).  Resident (num_kernels.hip): log-alpha and
// log-beta per state, y per unique (frame, pdf), the occupation per arc, of a whole sequence.  Windowed
// (num_windowed_kernels.hip): log-alpha and log-beta of two adjacent levels, y and the occupations of one frame.
inline size_t num_resident_lds_bytes(int32_t max_states, int32_t max_arcs, int32_t max_uniq) {
  return (size_t)((max_states + 1) & ~1) * 16 + (size_t)((max_uniq + 3) & ~3) * 4 + (size_t)((max_arcs + 3) & ~3) * 4;
}
inline size_t num_windowed_lds_bytes(int32_t level_states, int32_t level_arcs, int32_t frame_uniq) {
  return (size_t)((level_states + 1) & ~1) * 32 + (size_t)((frame_uniq + 3) & ~3) * 4 + (size_t)((level_arcs + 3) & ~3) * 4;
}
// (beside its dynamic arrays the windowed kernel has a total and the 128 shares of the cross-entropy sum in static LDS)
inline bool num_windowed_fits(size_t dynamic_bytes) { return dynamic_bytes + 2048 <= (size_t)kLdsLimitBytes; }

// End-to-end supervision ([K] Supervision::e2e_fsts, supervision_e2e.cpp): per-sequence acceptors with cycles, walked
// frame by frame by num_e2e_kernels.hip.  Per sequence: states [state_off[s], state_off[s+1]), arcs [arc_off[s], ...),
// distinct pdfs [pdf_off[s], ...).  An arc's key packs its other state (source for in-arcs, destination for out-arcs) in
// the low 16 bits and the sequence-local pdf number ("upid") in the high 16 bits; its weight is the log-probability
// -cost.  Out-arcs are sorted by source (the order of the input); an arc's posterior slot is its out-arc position.
struct E2eTables {
  std::vector<int32_t> state_off, arc_off, pdf_off, start;  // S + 1 (start: S)
  std::vector<int32_t> in_begin, out_begin;                 // per state + 1 per sequence, local arc positions
  std::vector<uint32_t> in_key, out_key;                    // per arc
  std::vector<float> in_lw, out_lw;                         // per arc: -cost
  std::vector<int32_t> pdf_begin, pdf_arc;                  // per upid + 1 per sequence; out-arc positions, increasing
  std::vector<int32_t> pdf_of;                              // per upid: the pdf (label - 1)
  std::vector<float> final_lw;                              // per state: -final cost, -inf when not final
  int32_t max_states = 0, max_arcs = 0, max_pdfs = 0;
  int64_t total_states = 0, total_pdfs = 0;
};

// bound on an e2e supervision's kernel scratch ((T + 1) x states x 8 + T x distinct pdfs x 4 bytes): tc_supervision_create_e2e
constexpr int64_t kE2eMaxScratchBytes = (int64_t)4 << 30;
struct E2eDev {
  const int32_t *state_off, *arc_off, *pdf_off, *start, *in_begin, *out_begin, *pdf_begin, *pdf_arc, *pdf_of;
  const uint32_t *in_key, *out_key;
  const float *in_lw, *out_lw, *final_lw;
  // scratch in the same pool slot, not uploaded: the log-alpha history (double) [(T + 1) x state] per sequence (at
  // (T + 1) * state_off[s]), and per (frame, upid) y from the forward pass, overwritten by the backward pass with
  // weight * posterior (stage, [T x upid] per sequence at T * pdf_off[s])
  double *alpha_hist;
  int32_t max_states, max_arcs, max_pdfs;
  // num_e2e_large_kernels.hip's arc occupations, one float per arc of every sequence (at arc_off[s]): scratch of the slot
  // behind the stage, this many 256-byte units behind alpha_hist; 0: the slot has none (the handle fits the resident
  // kernel and was staged without "force_num_e2e_large").  It fills the structure's tail padding: kernel arguments keep
  // their offsets.
  int32_t occ_off256;
};
static_assert(sizeof(E2eDev) == 15 * sizeof(void *) + 16, "E2eDev: NumParams' layout is part of the resident kernels' code");

// One slot of the per-device supervision pool (supervision.cpp): device blob, pinned staging of the same size,
// `ready` = the upload has landed, `done` = the last launch that reads the blob has finished.
struct PoolSlot {
  char *blob = nullptr, *host = nullptr;
  size_t cap = 0;
  hipEvent_t ready = nullptr, done = nullptr;
};

struct NumDev {
  const int32_t *seq_state_off, *seq_arc_off, *seq_uniq_off, *level_begin, *out_begin, *in_begin, *in_arc,
      *arc_src, *arc_dst, *arc_uniq, *uniq_t, *uniq_pdf, *uniq_begin, *uniq_arc;
  const float *arc_logw, *final_logw;
  // the level-windowed kernel's: frame_uniq as NumTables'; alpha_hist = its log-alpha history, one double per state of
  // every sequence, in the pool slot behind the tables (not uploaded)
  const int32_t *frame_uniq = nullptr;
  double *alpha_hist = nullptr;
  float *stage = nullptr;  // [unique (frame, pdf) entries of all sequences]: posteriors in transit (launch_num_scatter)
  PoolSlot *slot = nullptr;
  size_t upload_bytes = 0;  // of the slot's pinned staging, to be copied to the device
  bool uploaded = false;    // the copy has been enqueued (tc_supervision_prepare); staged only: tc_supervision_stage
  int e2e = 0;  // end-to-end supervision: launch_num / launch_num_scatter take num_e2e_kernels.hip with these tables
  E2eDev e2e_tab = {};
};

struct NumParams {
  NumDev t;
  const float *y;
  int64_t y_stride;
  float *deriv;
  int64_t deriv_stride;
  float *xent;
  int64_t xent_stride;
  double *seq_logprob;  // [S]
  int S, T, P;
  float weight;
  float deriv_scale = 1.f, xent_scale = 1.f;  // tc_chain_objf_and_grad: -1 and -xent_regularize (else 1, 1)
  // non-zero: the kernel leaves weight * posterior in t.stage instead of adding it to deriv / writing xent, so that
  // it can run beside the denominator (which writes every element of deriv); launch_num_scatter finishes the job
  int staged = 0;
  // Kaldi's cross-entropy objective sum(xent_output * xent_deriv) has as many non-zero terms as xent_deriv has: the
  // kernel that writes xent_deriv's entries multiplies each by its xent_output element and leaves the sequence's sum
  // (double) in seq_xent -- instead of a pass over both dense matrices (1.26 GB at C3).  Null: not wanted.
  const float *xent_out = nullptr;
  int64_t xent_out_stride = 0;
  double *seq_xent = nullptr;  // [S]
  // non-zero: xent / xent_out are the caller's (B, C, T) tensors, element (sequence, pdf, frame) -- the numerator touches
  // only its posteriors' entries, so the 3-D call needs no frame-major copy of either (tc_chain_step)
  int xent_bct = 0, xent_out_bct = 0, y_bct = 0;  // (y is read at the supervision's (frame, pdf) pairs only)
  int lds_states, lds_arcs, lds_uniq;
  int win_states, win_arcs, win_uniq;  // the same for one level / one frame (the level-windowed kernel's LDS arrays)
  // TC_DTYPE_* of y and xent_out when they are the caller's 16-bit (B, C, T) tensors (tc_chain_step_typed): the kernels
  // widen what they read; the 2-D pointers of this structure are always float32
  int elem = TC_DTYPE_F32;
  // per-row factor of the xent stores (tc_chain_step_weighted: Kaldi's deriv_weights, indexed by the frame-major row
  // t*S + s): xent[...] = xent_row_w[row] * (xent_scale * v).  seq_xent keeps summing the unweighted xent_scale * v, and
  // deriv is not weighted here.  Null: no factor.
  const float *xent_row_w = nullptr;
  // ragged supervision: [S] frames of each sequence (device, in the supervision's pool slot); T above is the
  // longest -- the tensors' and the scratch's T.  Null: uniform.  (Behind every older member, as DenParams::seq_frames: the
  // uniform kernels' argument offsets stay what they were.)
  const int32_t *seq_frames = nullptr;
  // ragged regular supervision: NumTables::seq_level_off on the device ([S + 1]); null otherwise
  const int32_t *seq_level_off = nullptr;
  // tc_supervision_best_path (num_best_path_kernels.hip): [S][T] the best path's pdf per frame (-1 in the padding and for a
  // sequence without a path), [S] its log score.  Null for every other launch.  (At the end, as the two above.)
  int32_t *best_pdf = nullptr;
  double *best_score = nullptr;
  // tc_chain_step_log_softmax (xent_softmax_kernels.hip): [rows][2] the row statistics (max, log(sum(exp(x - max)))) of
  // xent_out's rows, row = t*S + s.  The cross-entropy objective's term becomes xent_scale * v * (x - max - log sum): the
  // log-softmax of the row.  Null: the plain product.  (The last member: every older argument offset stays.)
  const float *xent_lse = nullptr;
};

}  // namespace tc

struct tc_supervision {
  float weight = 1.f;
  int32_t S = 0, T = 0, P = 0;
  bool e2e = false;  // tc_supervision_create_e2e: `e2e_tab` holds the tables, `tab` is empty
  tc::NumTables tab;
  tc::E2eTables e2e_tab;
  // tc_supervision_create_ragged / tc_supervision_create_e2e_ragged: the sequences' lengths (S entries, T above is the
  // longest); empty: uniform
  std::vector<int32_t> frames;
  int64_t total_frames = 0;        // their sum (S * T for a uniform handle)
  std::vector<size_t> blob_off;    // offsets of the tables inside a pool slot
  std::mutex mu;
  std::map<int, tc::NumDev> dev;
  std::map<int, const int32_t *> frames_dev;  // ragged: the lengths in the device's pool slot, behind the tables
  std::map<int, const int32_t *> level_off_dev;  // ragged regular: NumTables::seq_level_off, in the same slot
};

namespace tc {

int build_schedules(tc_den_graph *g);                                                  // den_graph.cpp
void build_general(tc_den_graph *g);                                                   // schedule_general.cpp
bool detect_tied(tc_den_graph *g, std::vector<char> *special);                         // schedule_owner.cpp
bool make_work_graph(tc_den_graph *g);                                                 // schedule_owner.cpp
// (count_only: fills fwd / bwd.padded_arcs and the layout alone -- what a candidate row cut would cost)
// (general: owner-computes schedules of a graph that is not chain-structured -- every arc, its pdf in the cell)
bool build_owner(tc_den_graph *g, const std::vector<char> &special, int max_row, bool count_only = false, bool general = false);  // schedule_owner.cpp
int arrange_half(const std::vector<std::vector<int64_t>> &lane_arcs, int steps, const int32_t *other,
                 const int32_t *pdf, std::vector<std::vector<int>> *pos_out);          // den_layout.cpp
// ... one gather per cell (tied schedules): step by step, a matching of lanes to banks that keeps the half-slot on its
// lower bound max(steps, most loaded bank).  pad_bank[l][k]: the bank a padding cell should gather from.
int arrange_half_matching(const std::vector<std::vector<int64_t>> &lane_arcs, int steps, const int32_t *other,
                          std::vector<std::vector<int>> *pos_out, std::vector<std::vector<int>> *pad_bank,
                          int *lower_bound);                                           // den_layout.cpp
inline int round4(int x) { return (x + 3) & ~3; }
// need_alpha (the general owner-computes kernel): only layouts with alpha' in LDS; when the frame sums of T_hint frames
// do not fit behind one, they go to the workspace (asum_global) instead of alpha' going to the history
bool compute_layout(int H, int P, int T_hint, int extra_slots, bool tied, DenLayout *L, bool need_alpha = false);
constexpr int asum_stride(int T) { return (T + 2 + 3) & ~3; }
bool compute_layout_planes(int Npos, int P, int T_hint, int extra_slots, DenLayout *L);
int64_t layout_lds_bytes(const DenLayout &L, int T);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device, size class) instead of before every
// launch: it is a driver call on the launch path of the hot loop.
hipError_t allow_dynamic_lds(const void *kernel, size_t lds_bytes);                    // den_graph.cpp
int launch_den(const DenParams &p, hipStream_t stream);
int launch_den_big(const DenParams &p, int accumulate, hipStream_t stream);
int launch_den_tied(const DenParams &p, int accumulate, hipStream_t stream);  // den_tied_kernel.hip
// whether launch_den_tied runs the call on the fused kernel's full-layout twin (den_tied_kernel.hip: the conditions)
bool tied_full_layout(const DenParams &p);
int launch_den_general_owner(const DenParams &p, int accumulate, hipStream_t stream);  // den_general_owner.hip
int launch_den_tied_planes(const DenParams &p, int accumulate, hipStream_t stream);  // den_tied_planes.hip
// ... two workgroups per sequence meeting in the middle (batches of at most half the CUs)
bool planes_mitm_fits(const DenParams &p);
int launch_den_tied_planes_mitm(const DenParams &p, int accumulate, hipStream_t stream);
// den_tied_split.hip: the backward recursion alone (to run beside a forward-only launch_den_tied), and the pass
// that forms gamma / the derivative from the two histories
int launch_den_tied_backward_only(const DenParams &p, hipStream_t stream);
int launch_den_tied_combine(const DenParams &p, int accumulate, int num_cus, hipStream_t stream);
bool split_bwd_fits(const DenLayout &L, int T);  // the backward-only kernel's and the combining pass's LDS fit one CU
constexpr int kSplitMaxSeq = 128;  // two CUs per sequence: batches of at most half the chip's CUs
// den_tied_pair.hip: two sequences per workgroup, the two recursions of a pair on two CUs meeting in the middle
int launch_den_tied_pair(const DenParams &p, int extra_slots, int accumulate, hipStream_t stream);
bool pair_fits(const DenLayout &L, int extra_slots, int T);
int tune_den_variant(tc_den_graph *g, int device);  // api.cpp
// tuning_cache.cpp: the measured choices of earlier runs, keyed by graph hash and device name
std::string tuning_cache_key(uint64_t graph_hash, const char *device_name);
bool tuning_cache_get(const std::string &key, int *two_sequence_kernel);
void tuning_cache_put(const std::string &key, int two_sequence_kernel, float fused_ms, float two_sequence_ms);
// den_tied_mitm.hip: two CUs per sequence meeting in the middle (batches of at most half the CUs)
int launch_den_tied_mitm(const DenParams &p, uint32_t *sync, int accumulate, hipStream_t stream);
bool mitm_fits(const DenLayout &L, int T);
size_t mitm_sync_bytes(int S);
int pair_norm_stride(int T);
size_t pair_sync_bytes(int S);
inline size_t pair_stamp_bytes(int T) { return ((size_t)2 * kWaves * (T + 2) * 8 * 8 + 255) & ~(size_t)255; }
int64_t big_small_floats(int hb, int P, int T, int Sp);
int launch_num(const NumParams &p, hipStream_t stream);
int launch_num_scatter(const NumParams &p, hipStream_t stream);
int launch_num_windowed(const NumParams &p, hipStream_t stream);     // num_windowed_kernels.hip (via launch_num)
int launch_num_e2e(const NumParams &p, hipStream_t stream);          // num_e2e_kernels.hip (via launch_num)
int launch_num_e2e_scatter(const NumParams &p, hipStream_t stream);  // ... (via launch_num_scatter)
int launch_num_best_path(const NumParams &p, hipStream_t stream);    // num_best_path_kernels.hip (regular and end-to-end)
int launch_den_best_path(const DenBestParams &p, hipStream_t stream);  // den_best_path_kernels.hip
int den_best_tables(tc_den_graph *g, int device, DenBestDev *out);   // den_graph.cpp: made and uploaded on first use
int launch_den_accuracy_rows(const DenAccRowParams &p, bool dense, hipStream_t stream);  // den_accuracy_kernels.hip
int launch_den_accuracy_grad(const DenAccGradParams &p, bool dense, hipStream_t stream);
int den_acc_tables(tc_den_graph *g, int device, DenAccDev *out);     // den_graph.cpp: made and uploaded on first use
int launch_den_sample_paths(const DenSampleParams &p, hipStream_t stream);  // den_sample_kernels.hip
int launch_path_edit(const PathEditParams &p, hipStream_t stream);      // path_edit_kernels.hip
int launch_sampled_risk_grad(const SampledRiskGradParams &p, int dtype, hipStream_t stream);
// dynamic LDS of num_e2e_kernel: two double score vectors, the frame's y per distinct pdf and one float per arc (max_arcs = 0:
// of the kernels that keep no arc occupations on chip, num_e2e_large_kernel and num_e2e_best_path_kernel)
inline size_t num_e2e_lds_bytes(int max_states, int max_arcs, int max_pdfs) {
  return (size_t)2 * ((max_states + 3) & ~3) * sizeof(double) + (((max_pdfs + 3) & ~3) + (size_t)max_arcs) * sizeof(float);
}
// num_e2e_large_kernels.hip: the end-to-end numerator for sequences beyond the resident kernel's TC_E2E_MAX_* (launch_num_e2e
// dispatches).  Its LDS is num_e2e_lds_bytes(states, 0, pdfs); e2e_large_fits is tc_supervision_create_e2e_any's size rule.
int launch_num_e2e_large(const NumParams &p, hipStream_t stream);
inline bool e2e_beyond_resident(int max_states, int max_arcs, int max_pdfs) {
  return max_states > TC_E2E_MAX_STATES || max_arcs > TC_E2E_MAX_ARCS || max_pdfs > TC_E2E_MAX_PDFS;
}
inline bool e2e_large_fits(int states, int pdfs) {
  return num_windowed_fits((size_t)16 * ((states + 3) & ~3) + (size_t)4 * ((pdfs + 3) & ~3));
}
// Dynamic LDS of a launch of num_e2e_large_kernel / num_e2e_best_path_kernel, which lay it out with each sequence's own
// sizes.  Every sequence of a handle meets e2e_large_fits (the create entries), so none needs more than the rule admits; none
// needs more than the batch's largest state count beside its largest pdf count either, which may belong to two sequences.
inline size_t e2e_seq_lds_bytes(int max_states, int max_pdfs) {
  const size_t both = num_e2e_lds_bytes(max_states, 0, max_pdfs), rule = (size_t)kLdsLimitBytes - 2048;
  return both < rule ? both : rule;
}
// Side streams and fork / join events per (device, caller stream) (made on first use; the hot path only records and waits):
// `den_side` carries the backward recursion of the two-CU form (den_tied_split.hip), `num_side` the numerator when
// the denominator leaves CUs idle (api.cpp).
struct SideStreams {
  hipStream_t den_side = nullptr, num_side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, num_fork = nullptr, num_join = nullptr;
  int num_cus = 0;
  std::recursive_mutex enqueue;  // one caller at a time records / waits on the events (a wait binds to the latest record)
};
int side_streams(hipStream_t stream, SideStreams **out);  // den_graph.cpp
void side_streams_forget(hipStream_t stream);              // ... before a caller stream is destroyed
// CUs a denominator launch of S sequences occupies (two per sequence in the two-CU form, all for the streamed path)
int den_cus_used(const DenParams &p, int num_cus);
bool den_zeroes_xent(const DenParams &p, int num_cus);  // whether the kernel launch_den_mode will take honours xent_zero
// (total_frames: a ragged minibatch's sum of lengths, the objective's weight is sup_weight times it; 0: S * T)
int launch_finalize(const double *den_lp, const double *num_lp, const double *y2, const float *ab, const float *gs,
                    int S, int T, float sup_weight, float l2, int have_deriv, float *results, int32_t *fail_flag,
                    hipStream_t stream, const double *xent_lp = nullptr, double *xent_total = nullptr,
                    float *loss_out = nullptr, int64_t total_frames = 0);
// The finalize of tc_chain_step_per_sequence (a sibling kernel: finalize_kernel keeps its instruction stream).  Forms each
// sequence's status (1: numerator, 2: denominator, 4: alpha-beta check non-finite), writes seq_results ([S][6] doubles:
// num_lp, den_lp, y2, xent sum, frames, status; nullable) and alive_frames ([S]: the sequence's own frames, or 0 when it is
// masked out).  isolate: the sums run over the sequences of status 0, in finalize_kernel's order, a masked term being an
// exact +0.0, and the alpha-beta sums are held against their count.  When nothing failed, everything failed or the
// survivors miss that check, the unmasked sums give finalize_kernel's outputs bit for bit and alive_frames holds every
// sequence's own length.  seq_frames: a ragged minibatch's lengths (null: T each).
int launch_finalize_per_sequence(const double *den_lp, const double *num_lp, const double *y2, const float *ab, const float *gs,
                                 int S, int T, float sup_weight, float l2, int have_deriv, float *results, int32_t *fail_flag,
                                 hipStream_t stream, const double *xent_lp, double *xent_total, float *loss_out,
                                 int64_t total_frames, const int32_t *seq_frames, int isolate, double *seq_results,
                                 int32_t *alive_frames);
// ... its zeroing: +0 into frames >= alive_frames[b] of sequence b, as launch_zero_padding but from frame 0 where
// alive_frames[b] is 0 (a failed sequence is a sequence of no frames)
int launch_zero_failed(void *out, int elem_bytes, int64_t sb, int64_t st, int64_t sc, int B, int T, int cols,
                       const int32_t *alive_frames, hipStream_t stream);
// Ragged minibatches: +0 into the elements of frames >= seq_frames[b] of an output tensor whose element (b, t, c) lies at
// b*sb + t*st + c*sc (element strides; elem_bytes 4 or 2) -- every layout and dtype of the entries; costs what the padding
// costs.  (layout_rows_kernels.hip)
int launch_zero_padding(void *out, int elem_bytes, int64_t sb, int64_t st, int64_t sc, int B, int T, int cols,
                        const int32_t *seq_frames, hipStream_t stream);
int launch_zero_on_fail(const int32_t *fail_flag, float *a, int64_t a_stride, float *b, int64_t b_stride,
                        const float *y, int64_t y_stride, float l2_scale, int64_t rows, int cols, hipStream_t stream);
int launch_den_reduce(const double *den_lp, const float *ab, const float *gs, int S, double *logprob_out,
                      int32_t *status_out, hipStream_t stream);
int launch_sum_double(const double *in, int n, double scale, double *out, hipStream_t stream);
int launch_xent_total(const double *in, int n, const int32_t *fail_flag, double *out, hipStream_t stream);
int launch_step_loss(const float *results3, float *loss1, hipStream_t stream);
int64_t trace_workspace_bytes();
int launch_trace_mat_mat(const float *a, int64_t a_stride, const float *b, int64_t b_stride, int64_t rows, int cols,
                         double *partial, double *out, hipStream_t stream);
// The one limit of the network output: the denominator kernels take exp(y) at clamp(y, -kOutputLimit, kOutputLimit)
// (den_device.h:72-73, den_tied_device.h:83, den_slab_kernel.hip:47-48 spell the value out), and the out-of-range penalty
// of tc_chain_step_penalized (after [K] PenalizeOutOfRange, restated in torchain_hip.h) acts outside the same range.
constexpr float kOutputLimit = 30.0f;
// The passes that write a gradient last -- the (B, C, T) copy back, the 16-bit rounding pass, the in-place float32 row
// pass and the channel-last scatter -- and what each is told.  Every element leaves as half_io.h's last_elem states it:
//   scale * v;  with row_w, (scale * row_w[row]) * v in one multiply (tc_chain_step_weighted);
//   with pen_c2 = fl32(2 * c) > 0 (tc_chain_step_penalized), row_w[row] * penalize(scale * v, y), row_w NULL taken as 1,
//   an element whose y lies in range keeping the bits of scale * v.
// y is the network output of the element, laid out as the pass's OUTPUT is: the caller's (B, C, T) tensor of `dtype`; the
// n contiguous widened floats; float32 rows of y_stride; or a channel-last view of `dtype` with batch stride y_stride and
// frame stride y_st.  !scaled (the scatter alone): the values are final and are only moved and rounded.
struct LastPass {
  float scale = 1.0f;
  const float *row_w = nullptr;
  float pen_c2 = 0.0f;
  const void *y = nullptr;
  int64_t y_stride = 0, y_st = 0;
  bool scaled = true;
};
// layout_kernels.hip.  The tiled copies between a (B, C, T) tensor of `dtype` (TC_DTYPE_*) and frame-major float32 rows;
// layout_grid_ok: whether their grid takes B sequences of T frames (else TC_ERR_UNSUPPORTED)
bool layout_grid_ok(int B, int T);
int launch_to2d(int dtype, const void *in_bct, float *out, int B, int Cn, int T, int64_t stride2d, hipStream_t stream);
int launch_from2d(int dtype, const float *in, int64_t stride2d, void *out_bct, int B, int Cn, int T, const LastPass &lp,
                  hipStream_t stream);
// 16-bit 2-D tensors (TC_DTYPE_BF16 / TC_DTYPE_F16 only): the widening copy of strided rows into a contiguous float32
// matrix, and the rounding copy of n contiguous floats, `cols` a row (read with row_w only), whose sign is final (scale 1)
int launch_widen_rows(int dtype, const void *in, int64_t in_stride, float *out, int64_t rows, int cols, hipStream_t stream);
int launch_round(int dtype, const float *in, void *out, int64_t n, int cols, const LastPass &lp, hipStream_t stream);
// in place on a contiguous float32 (rows, cols) matrix whose sign is final (scale 1): the 2-D float32 MMI gradient, which
// the denominator and the numerator write straight into the caller's tensor.  Needs row_w or the penalty.
int launch_scale_rows(float *a, int64_t rows, int cols, const LastPass &lp, hipStream_t stream);
// layout_rows_kernels.hip (tc_chain_step_strided, TC_LAYOUT_CHANNEL_LAST): the row copies of a channel-last view, element
// (b, c, t) at b*sb + t*st + c in a tensor of `dtype`.  Strides of size-1 dimensions are ignored; rows must not overlap.
bool channel_last_strides_ok(int B, int T, int cols, int64_t sb, int64_t st);
// out[(t*B + b) * out_stride + c] = widen(x[b*sb + t*st + c])
int launch_rows_gather(int dtype, const void *x, int64_t sb, int64_t st, float *out, int64_t out_stride, int B, int T, int cols,
                       hipStream_t stream);
// out[b*osb + t*ost + c] = in[(t*B + b) * in_stride + c] on its way out, rounded once
int launch_rows_scatter(int dtype, const float *in, int64_t in_stride, void *out, int64_t osb, int64_t ost, int B, int T,
                        int cols, const LastPass &lp, hipStream_t stream);

// xent_softmax_kernels.hip (tc_chain_step_log_softmax): the cross-entropy head's log-softmax folded into the step.  x is
// xent_input where the step's table puts it: float32 rows with unit channel stride (x_bct == 0: row t*S + s at
// row * x_stride), or the caller's (B, C, T) tensor of `dtype` (x_bct != 0).  stats: [S*T][2] floats, row t*S + s.
// launch_xent_row_stats leaves (max, log(sum(exp(x - max)))) of every row.  launch_xent_softmax_grad turns the xent
// gradient V the numerator left in g (rows of g_stride, or a float32 (B, C, T) tensor) into V - rowsum(V) * softmax(x) in
// place; a row without a non-zero entry of V becomes +0 by a select.  live_frames ([S], nullable): rows of frames >=
// live_frames[s] are left alone (padding, and the failed sequences of the isolating step).
int launch_xent_row_stats(int dtype, const void *x, int x_bct, int64_t x_stride, int S, int T, int P, float *stats,
                          hipStream_t stream);
int launch_xent_softmax_grad(int dtype, const void *x, int x_bct, int64_t x_stride, float *g, int64_t g_stride, int S, int T,
                             int P, const float *stats, const int32_t *live_frames, hipStream_t stream);

// boost_kernels.hip (tc_chain_step_boosted, tc_boost_rows): the denominator's private matrix y_b = fl32(y - fl32(b * a)) of
// boosted LF-MMI, and the fix-up that keeps the l2 term on the true y.  BoostAcc is a_t(j) in one of its two forms -- the
// hard reference (ref: [S * T], entry s * T + t; cls: nullable [P]) or the dense matrix (acc: row t*S + s, acc_stride floats
// apart) -- with b = fl32(boost) and the lengths of a ragged batch (nullable): rows of frames >= seq_frames[s] read neither.
struct BoostAcc {
  const int32_t *ref = nullptr, *cls = nullptr;
  const float *acc = nullptr;
  int64_t acc_stride = 0;
  float b = 0.0f;
  const int32_t *seq_frames = nullptr;
};
// out[(t*S + s) * out_stride + c] = boosted(widen(x[s*sb + t*st + c])): rows with unit channel stride of `dtype`
int launch_boost_rows(int dtype, const void *x, int64_t sb, int64_t st, float *out, int64_t out_stride, int S, int T, int cols,
                      const BoostAcc &a, hipStream_t stream);
// ... the same from a contiguous (B, C, T) tensor of `dtype` (layout_grid_ok's limits)
int launch_boost_bct(int dtype, const void *in_bct, float *out, int64_t out_stride, int B, int Cn, int T, const BoostAcc &a,
                     hipStream_t stream);
// seq_y2[s] += sum(2 * y_b * d + d^2) and g -= l2_scale * d over the live elements with d = fl32(b * a) != 0
int launch_boost_l2_sum(const float *yb, int64_t yb_stride, int S, int T, int P, const BoostAcc &a, double *seq_y2,
                        hipStream_t stream);
int launch_boost_l2_grad(float *g, int64_t g_stride, int S, int T, int P, const BoostAcc &a, float l2_scale, hipStream_t stream);

extern thread_local int g_last_hip_error;

// Diagnostic switches (tc_debug_set in the public header): process-wide, read when a graph is built.  They
// replace what used to be environment variables of the shipping library.
// bumped whenever a round changes a kernel the per-graph choice is timed on (tuning_cache.cpp: part of the cache key)
constexpr int kKernelGeneration = 6;
enum DebugFlag { kDbgForceGeneral = 0, kDbgForceStreamed, kDbgNoSplit, kDbgNoPdfBanks, kDbgNoBankSearch, kDbgSchedTrace, kDbgNoPhaseSplit, kDbgNoNumOverlap, kDbgNoPair, kDbgForcePair, kDbgNoTune, kDbgNoMitm, kDbgForceMitm, kDbgSlabWide, kDbgSlabNarrow, kDbgExpPerFrame, kDbgOldArrange, kDbgNoPlanes, kDbgOldGeneral, kDbgPhantomPdf0, kDbgNoPdfSearch, kDbgNoSplitSrc, kDbgPlanesMeetAt, kDbgForceNumWindowed, kDbgForceDenBestStreamed, kDbgForceNumE2eLarge, kDbgNoFullLayout, kDbgForceDenAccStreamed, kDbgForceDenSampleStreamed, kDbgCount };
bool debug_flag(DebugFlag f);
int debug_value(DebugFlag f);  // the switch's integer value (0: not set)

int pool_acquire(int device, size_t bytes, PoolSlot **out);                      // supervision.cpp
void pool_release(int device, PoolSlot *slot);
int64_t pool_counter(int which);  // 0: device allocations made by the pool, 1: slots reused
// launches enqueued so far, by kind (tc_debug_counter): the evaluation-step tests read them to see that a forward-only
// call enqueued no backward recursion
enum LaunchCounter { kCntDen = 0, kCntDenBackward, kCntNum, kCntNumBackward, kCntLayout, kCntDenAsumGlobal, kCntNumE2eStaged, kCntNumWindowed, kCntChannelLast, kCntRagged, kCntRaggedTwoCu, kCntBestPath, kCntDenBestPath, kCntDenBestPathStreamed, kCntXentLogSoftmax, kCntNumE2eLarge, kCntTiedFullLayout, kCntDenAccuracy, kCntDenAccuracyGrad, kCntDenAccuracyGradStreamed, kCntDenAccuracyDense, kCntDenAccuracyDenseGrad, kCntDenSample, kCntDenSampleStreamed, kCntPathEdit, kCntSampledRiskGrad, kCntBoost, kCntCount };
void count_launch(LaunchCounter c);
int supervision_mark_use(tc_supervision *sup, int device, hipStream_t stream);
int stage_e2e_locked(tc_supervision *sup, int device);  // supervision_e2e.cpp (caller holds sup->mu)
int supervision_from_example(const tc_example *ex, tc_supervision **out);  // egs_reader.cpp: regular or e2e
#define TC_HIP_CHECK(expr)                        \
  do {                                            \
    hipError_t e__ = (expr);                      \
    if (e__ != hipSuccess) {                      \
      tc::g_last_hip_error = (int)e__;            \
      return TC_ERR_HIP;                          \
    }                                             \
  } while (0)

}  // namespace tc
