// C ABI entry points of the hot path (include/torchain_hip.h).  Replaces the reference's Kaldi
// bridge src/my_lib_chain.cpp:104-136: validates the borrowed tensors the way common::make_matrix
// does (2-D, unit column stride, src/common.hpp:109-117), carves the caller's workspace, and enqueues
// the kernels on the caller's stream.  No host synchronisation; no allocation once the per-device supervision
// pool (supervision.cpp) is warm.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <string>
#include <cstring>

#include "chain_internal.h"

using namespace tc;

namespace tc {
int launch_den_mode(const DenParams &p, int accumulate, hipStream_t stream);
}

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Workspace {
  float *big_expy, *big_beta, *big_small, *big_y;  // streamed path only
  uint32_t *big_gam = nullptr;
  int big_exp_frames = 1;
  float *beta_hist, *fwd_norm, *bwd_norm;          // two-CU forms of small batches only (den_tied_split.hip, den_tied_mitm.hip)
  uint32_t *mitm_sync = nullptr;
  float *pair_norm = nullptr;                      // two-sequence form (den_tied_pair.hip)
  uint32_t *pair_sync = nullptr;
  long long *pair_stamps = nullptr;                // ... its diagnostic builds (-DTC_PAIR_STAMPS): raw cycle stamps
  float *alpha_hist, *asum_g;
  float *src_scratch = nullptr, *part_scratch = nullptr;  // plane-wise kernel with a split gather source (28673..40960 positions)
  double *den_lp, *num_lp, *y2, *xent_lp;
  float *ab, *gs;
  int32_t *fail;
  int32_t *alive_frames;  // per sequence, its own frames or 0 for a failed one: the isolating step (tc_chain_step_per_sequence)
  double *scalar;
  size_t total;
};

// Hs: stored states per frame of the alpha history (layout positions for tied graphs: build_owner)
int hist_states(const tc_den_graph *g) {
  if (g->big) return ((g->tied ? g->work_H : g->H) + 3) & ~3;
  return g->tied || g->gen_owner ? g->layout.Hs : ((g->H + 3) & ~3);
}
int big_p(const tc_den_graph *g) { return g->big ? g->P : 0; }
int big_h(const tc_den_graph *g) { return g->big ? (g->tied ? g->work_H : g->H) : 0; }  // tied: work-graph states
int big_g(const tc_den_graph *g) { return g->big ? g->big_G : 16; }
int big_hb(const tc_den_graph *g) { return g->big ? g->big_hb : 0; }
// Batches the tied on-chip kernel may run as two CUs per sequence get room for the second history.  (Whether
// they do is decided at launch: device size, layout for this T, diagnostic switch.)
bool split_room(const tc_den_graph *g, int S) { return g->tied && !g->big && S <= kSplitMaxSeq; }
// Tied on-chip graphs of at most 8192 positions may run two sequences per workgroup (den_tied_pair.hip): two more
// history rows, the two roles' normalisers and the pairing words.
// ... the plane-wise kernel of 16385..40960 positions (den_tied_planes.hip): scratch rows of its split-source form
bool planes_room(const tc_den_graph *g) { return g->tied && !g->big && g->layout_ok && g->layout.planewise; }
bool pair_room(const tc_den_graph *g) { return g->tied && !g->big && g->layout_ok && g->layout.JV == kJvSmall; }

// big_P != 0 selects the streamed path's layout: sequences padded to slabs of 16, [slab][state][16] matrices
Workspace carve(char *base, int Hs, int S, int T, int big_P = 0, int big_H = 0, int big_G = 16, int big_hb = 0, bool split = false, bool pair = false,
                bool planes = false) {
  Workspace w;
  const int Sp = (S + big_G - 1) / big_G * big_G;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  // (pair form: row T + 1 holds the backward role's B_M)
  w.alpha_hist = (float *)take(big_P ? (size_t)(T + 1) * Sp * big_H * sizeof(float) : (size_t)(T + (pair ? 2 : 1)) * S * Hs * sizeof(float));
  w.asum_g = (float *)take((size_t)S * asum_stride(T) * sizeof(float));  // frame sums of utterances too long for LDS
  if (planes && Hs > kMaxPlanePositions) {
    const int planes_n = Hs / 4096, planes_b = planes_n - (planes_n + 1) / 2;
    // (per WORKGROUP: two per sequence in the two-workgroup form of small batches)
    w.src_scratch = (float *)take((size_t)2 * S * 4096 * planes_b * sizeof(float));
    w.part_scratch = (float *)take((size_t)2 * S * (Hs + 4096 * ((planes_n + 1) / 2)) * sizeof(float));  // (+ alpha' of the first half's planes)
  }
  w.den_lp = (double *)take((size_t)S * 8);
  w.num_lp = (double *)take((size_t)S * 8);
  w.xent_lp = (double *)take((size_t)S * 8);
  w.y2 = (double *)take((size_t)S * 8);
  w.ab = (float *)take((size_t)S * 4);
  w.gs = (float *)take((size_t)S * 4);
  w.fail = (int32_t *)take(256);
  w.alive_frames = (int32_t *)take((size_t)S * 4);
  w.scalar = (double *)take(4096);  // also the stamp area of diagnostic builds
  // streamed path: exp(y) of every frame, transposed once and used by both passes, when that is at most 1 GB
  // (else one frame at a time, recomputed by the backward pass: 2-7 % slower, measured; the cap keeps the workspace
  // of exactly the largest graphs from growing by gigabytes -- include/torchain_hip.h states the sizes)
  // (the diagnostic switch exp_per_frame selects the one-frame form at LAUNCH; the workspace is sized for the larger
  // layout whatever the switch says, so a size a caller cached stays valid when the switch changes)
  const int exp_frames_room = big_P && (size_t)T * Sp * big_P * sizeof(float) <= ((size_t)1 << 30) ? T : 1;
  w.big_exp_frames = debug_flag(kDbgExpPerFrame) ? 1 : exp_frames_room;
  w.big_expy = big_P ? (float *)take((size_t)exp_frames_room * Sp * big_P * sizeof(float)) : nullptr;
  w.big_beta = big_P ? (float *)take((size_t)2 * Sp * big_H * sizeof(float)) : nullptr;
  w.big_small = big_P ? (float *)take((size_t)big_small_floats(big_hb, big_P, T, Sp) * sizeof(float)) : nullptr;
  w.big_y = big_P ? (float *)take((size_t)Sp * big_H * sizeof(float)) : nullptr;
  w.big_gam = big_P ? (uint32_t *)take((size_t)Sp * big_P * sizeof(uint32_t)) : nullptr;
  w.beta_hist = split ? (float *)take((size_t)(T + 1) * S * Hs * sizeof(float)) : nullptr;
  w.fwd_norm = split ? (float *)take((size_t)S * (T + 2) * sizeof(float)) : nullptr;
  w.bwd_norm = split ? (float *)take((size_t)S * (T + 1) * sizeof(float)) : nullptr;
  w.mitm_sync = split ? (uint32_t *)take(mitm_sync_bytes(S)) : nullptr;
  w.pair_sync = pair ? (uint32_t *)take(pair_sync_bytes(S)) : nullptr;
  w.pair_norm = pair ? (float *)take((size_t)2 * (S + 1) * pair_norm_stride(T) * sizeof(float)) : nullptr;  // (+ a spare row each)
  w.pair_stamps = pair ? (long long *)take(pair_stamp_bytes(T)) : nullptr;  // (the workspace's last block)
  w.total = off;
  return w;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) ok = false;
    if (ok && prev != device && hipSetDevice(device) != hipSuccess) ok = false;
    if (prev == device) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int fill_den_params(tc_den_graph *g, int device, int32_t S, const float *y, int64_t rows, int32_t cols,
                    int64_t y_stride, float leaky, float deriv_weight, float l2_scale, float *deriv,
                    int64_t deriv_stride, const Workspace &w, DenParams *p, const DenGraphDev *tuning = nullptr,
                    const int32_t *seq_frames = nullptr) {
  if (!g || !y || S <= 0 || rows <= 0 || rows % S != 0) return TC_ERR_INVALID_ARGUMENT;
  // a ragged batch on a graph of the streamed path (lanes run over sequences: one frame count), before anything is launched
  if (seq_frames && g->big) return TC_ERR_UNSUPPORTED;
  if (cols != g->P || y_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (deriv && deriv_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (!(leaky > 0.0f && leaky < 1.0f)) return TC_ERR_INVALID_ARGUMENT;  // [K] KALDI_ASSERT in the ctor
  const int T = (int)(rows / S);
  DenGraphDev d;
  if (tuning) {
    d = *tuning;  // (tune_den_variant: the variant under test is in its pair_choice)
  } else {
    int rc = tc_den_graph_prepare(g, device);
    if (rc != TC_OK) return rc;
    std::lock_guard<std::mutex> lock(g->mu);
    d = g->dev[device];
  }
  bool tied = g->tied;
  // tied graphs address states by layout position (a multiple of 4096 of them, phantoms included)
  const int nstates = g->big ? (tied ? g->work_H : g->H) : (tied || g->gen_owner ? g->layout.Hs : g->H);
  if (g->big) {
    p->L = DenLayout();
    p->L.Hs = (nstates + 3) & ~3;
    p->L.Ps = (g->P + 3) & ~3;
    tied = false;  // the on-chip tied kernel's tables are not used; p->big.tied selects the streamed variant
  } else if (g->layout.planewise ? !compute_layout_planes(nstates, g->P, T, std::max(g->fwd.extra_slots, g->bwd.extra_slots), &p->L)
                                 : !compute_layout(nstates, g->P, T, std::max(g->fwd.extra_slots, g->bwd.extra_slots), tied, &p->L, g->gen_owner)) {
    return TC_ERR_UNSUPPORTED;  // decided at graph build with T = 256; a much longer T may not fit LDS
  }
  p->big = d.big;
  p->big_expy = w.big_expy;
  p->big_exp_stride = w.big_exp_frames > 1 ? (int64_t)((S + g->big_G - 1) / g->big_G * g->big_G) * g->P : 0;
  p->big_beta = w.big_beta;
  p->big_small = w.big_small;
  p->big_y = w.big_y;
  p->big_gam = w.big_gam;
  p->beta_hist = w.beta_hist;
  p->fwd_norm = w.fwd_norm;
  p->bwd_norm = w.bwd_norm;
  p->mitm_sync = w.mitm_sync;
  p->pair_norm = w.pair_norm;
  p->pair_sync = w.pair_sync;
  p->pair_stamps = w.pair_stamps;
  p->pair_extra_slots = std::max(g->fwd.extra_slots, g->bwd.extra_slots);
  p->pair_choice = d.pair_choice > 0 ? 1 : 0;
  p->big_Sp = (S + g->big_G - 1) / g->big_G * g->big_G;
  p->big_sum_pi = g->big_sum_pi;
  p->gen_owner = !g->big && g->gen_owner ? 1 : 0;
  p->tied_fs = tied ? d.tied_fs : nullptr;
  p->tied_w = tied ? d.tied_w : nullptr;
  p->fwd = d.fwd;
  p->bwd = d.bwd;
  p->pi = d.pi;
  p->y = y;
  p->y_stride = y_stride;
  p->deriv = deriv;
  p->deriv_stride = deriv_stride;
  p->alpha_hist = w.alpha_hist;
  p->asum_g = w.asum_g;
  p->src_scratch = w.src_scratch;
  p->part_scratch = w.part_scratch;
  p->seq_logprob = w.den_lp;
  p->seq_y2 = w.y2;
  p->seq_ab = w.ab;
  p->seq_gsum = w.gs;
  p->S = S;
  p->T = T;
  p->H = nstates;
  p->P = g->P;
  p->leaky = leaky;
  p->deriv_weight = deriv_weight;
  p->l2_scale = l2_scale;
  p->stamps = (long long *)w.scalar;
  p->y_vec = (cols % 4 == 0 && y_stride % 4 == 0 && aligned16(y)) ? 1 : 0;
  p->d_vec = (deriv && cols % 4 == 0 && deriv_stride % 4 == 0 && aligned16(deriv)) ? 1 : 0;
  p->set_seq_frames(seq_frames);
  return TC_OK;
}

int fill_num_params(tc_supervision *sup, int device, hipStream_t stream, const float *y, int64_t rows, int32_t cols,
                    int64_t y_stride, float *deriv, int64_t deriv_stride, float *xent, int64_t xent_stride,
                    double *seq_lp, NumParams *p) {
  if (!sup || !y) return TC_ERR_INVALID_ARGUMENT;
  if ((int64_t)sup->S * sup->T != rows || sup->P != cols || y_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if ((deriv && deriv_stride < cols) || (xent && xent_stride < cols)) return TC_ERR_INVALID_ARGUMENT;
  int rc = tc_supervision_prepare(sup, device, stream);
  if (rc != TC_OK) return rc;
  {
    std::lock_guard<std::mutex> lock(sup->mu);
    p->t = sup->dev[device];
    if (!sup->frames.empty()) {  // (in the same pool slot, uploaded with the tables)
      p->seq_frames = sup->frames_dev[device];
      if (!sup->e2e) p->seq_level_off = sup->level_off_dev[device];
    }
  }
  p->y = y;
  p->y_stride = y_stride;
  p->deriv = deriv;
  p->deriv_stride = deriv_stride;
  p->xent = xent;
  p->xent_stride = xent_stride;
  p->seq_logprob = seq_lp;
  p->S = sup->S;
  p->T = sup->T;
  p->P = sup->P;
  p->weight = sup->weight;
  p->lds_states = (sup->tab.max_states + 1) & ~1;
  p->lds_arcs = (sup->tab.max_arcs + 3) & ~3;
  p->lds_uniq = (sup->tab.max_uniq + 3) & ~3;
  p->win_states = (sup->tab.max_level_states + 1) & ~1;
  p->win_arcs = (sup->tab.max_level_arcs + 3) & ~3;
  p->win_uniq = (sup->tab.max_frame_uniq + 3) & ~3;
  return TC_OK;
}


}  // namespace

namespace tc {

// Fused kernel or two-sequence kernel for this graph on this device?  Both are run on a zero-filled batch of one
// sequence per CU and kTuneFrames frames (their time does not depend on the values) in scratch memory that is freed
// again; the two-sequence kernel is kept when it is at least 3% faster.  Any failure here leaves the fused kernel.
constexpr int kTuneFrames = 48, kTuneWarmup = 60, kTuneRounds = 4;
constexpr double kPairMinArcsPerState = 11.0;

int tune_den_variant(tc_den_graph *g, int device) {
  DenGraphDev d;
  {
    std::lock_guard<std::mutex> lock(g->mu);
    DenGraphDev &slot = g->dev[device];
    if (slot.pair_choice != -1) return TC_OK;
    slot.pair_choice = -2;  // (a concurrent caller runs the fused kernel meanwhile)
    d = slot;
  }
  int choice = 0;
  float ms[2] = {0.f, 0.f};
  int preset = -1;
  {
    std::lock_guard<std::mutex> lock(g->mu);
    auto it = g->preset_variant.find(device);
    if (it != g->preset_variant.end()) preset = it->second;
  }
  auto finish = [&]() {
    std::lock_guard<std::mutex> lock(g->mu);
    DenGraphDev &slot = g->dev[device];
    slot.pair_choice = choice;
    slot.tune_ms[0] = ms[0];
    slot.tune_ms[1] = ms[1];
    return TC_OK;
  };
  if (!pair_room(g) || !d.fwd.cells_pair || debug_flag(kDbgNoPair) || debug_flag(kDbgNoTune) || debug_flag(kDbgForcePair))
    return finish();
  // The two-sequence kernel shares one walk between two sequences and pays for it in its gamma frames: measured, it never
  // wins below about 11-12 arcs per state (C3's 8: 8 % slower) -- such graphs keep the fused kernel without being timed
  // (no timing launches, no scratch).  Its frame bodies are its own statement of the tied frame (clamp, gamma scale and
  // fixed-point adds are den_tied_device.h's shared helpers); tests/test_gpu_tied.py holds it to the fused kernel's values.
  if ((double)g->work_src.size() < kPairMinArcsPerState * (double)std::max(1, g->work_H) && preset < 0) return finish();
  if (preset >= 0) {  // the caller's choice (a cache of an earlier run, or rank 0's): no timing launches
    choice = preset;
    return finish();
  }
  // the choice an earlier run measured for this graph on this kind of device: no timing launches, no scratch allocation
  std::string cache_key;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) cache_key = tuning_cache_key(tc_den_graph_hash(g), prop.name);
    int cached = 0;
    if (!cache_key.empty() && tuning_cache_get(cache_key, &cached)) {
      choice = cached;
      return finish();
    }
  }
  DeviceGuard guard(device);
  if (!guard.ok) return finish();
  int num_cus = 0;
  if (hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || num_cus < 2)
    return finish();
  const int S = num_cus & ~1, T = kTuneFrames, P = g->P;
  const Workspace w0 = carve(nullptr, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g));
  const size_t ybytes = (size_t)S * T * P * sizeof(float);
  char *mem = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool ok = hipMalloc((void **)&mem, 2 * ybytes + w0.total + 512) == hipSuccess;
  ok = ok && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
  ok = ok && hipMemsetAsync(mem, 0, 2 * ybytes + w0.total + 512, stream) == hipSuccess;
  if (ok) {
    float *y = (float *)mem, *deriv = (float *)(mem + ybytes);
    char *wsp = mem + 2 * ybytes;
    wsp += (256 - ((uintptr_t)wsp & 255)) & 255;
    const Workspace w = carve(wsp, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g));
    DenParams p[2];
    for (int variant = 0; variant < 2 && ok; ++variant) {
      d.pair_choice = variant;
      ok = fill_den_params(g, device, S, y, (int64_t)S * T, P, P, 0.1f, -1.0f, 0.f, deriv, P, w, &p[variant], &d) == TC_OK;
    }
    // Untimed launches until the clocks have settled (a graph usually arrives on an idle device), then the two
    // kernels in turn, the best of kRounds each.
    for (int i = 0; i < kTuneWarmup && ok; ++i) ok = launch_den_mode(p[i & 1], 0, stream) == TC_OK;
    ms[0] = ms[1] = 1e30f;
    for (int round = 0; round < kTuneRounds && ok; ++round)
      for (int variant = 0; variant < 2 && ok; ++variant) {
        float t = 0.f;
        ok = hipEventRecord(e0, stream) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i) ok = launch_den_mode(p[variant], 0, stream) == TC_OK;
        ok = ok && hipEventRecord(e1, stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
        ok = ok && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
        ms[variant] = std::min(ms[variant], 0.5f * t);
      }
    if (!ok) ms[0] = ms[1] = 0.f;
    if (ok && ms[1] < 0.97f * ms[0]) choice = 1;
  }
  if (stream) (void)hipStreamSynchronize(stream);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (stream) {
    side_streams_forget(stream);  // (launch_den_mode made an entry for the temporary stream)
    (void)hipStreamDestroy(stream);
  }
  if (mem) (void)hipFree(mem);
  (void)hipGetLastError();  // (a failed scratch allocation is not the caller's error)
  if (ms[0] > 0.f && ms[1] > 0.f && !cache_key.empty()) tuning_cache_put(cache_key, choice, ms[0], ms[1]);  // (really timed)
  return finish();
}

}  // namespace tc

extern "C" {

int tc_den_graph_tuning(tc_den_graph *g, int device, int32_t *two_sequence_kernel, float *fused_ms, float *two_sequence_ms) {
  if (!g) return TC_ERR_INVALID_ARGUMENT;
  const int rc = tc_den_graph_prepare(g, device);
  if (rc != TC_OK) return rc;
  std::lock_guard<std::mutex> lock(g->mu);
  const DenGraphDev &d = g->dev[device];
  if (two_sequence_kernel) *two_sequence_kernel = d.pair_choice > 0 ? 1 : 0;
  if (fused_ms) *fused_ms = d.tune_ms[0];
  if (two_sequence_ms) *two_sequence_ms = d.tune_ms[1];
  return TC_OK;
}

int tc_den_graph_set_variant(tc_den_graph *g, int device, int32_t two_sequence_kernel) {
  if (!g || two_sequence_kernel < -1 || two_sequence_kernel > 1) return TC_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(g->mu);
  if (two_sequence_kernel < 0)
    g->preset_variant.erase(device);
  else
    g->preset_variant[device] = two_sequence_kernel;
  auto it = g->dev.find(device);
  if (it != g->dev.end() && it->second.pair_choice != -2) {
    // already on the device: the choice applies from the next launch on (-1: timed again at the next prepare); a graph
    // the two-sequence kernel does not fit keeps the fused one whatever is asked
    const bool fits = pair_room(g) && it->second.fwd.cells_pair;
    it->second.pair_choice = two_sequence_kernel < 0 ? -1 : (fits ? two_sequence_kernel : 0);
  }
  return TC_OK;
}

uint64_t tc_den_graph_hash(const tc_den_graph *g) {
  if (!g) return 0;
  // FNV-1a over what the schedules are built from: sizes, arcs (source, destination, pdf, probability bits)
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  mix(&g->H, sizeof(g->H));
  mix(&g->P, sizeof(g->P));
  mix(&g->A, sizeof(g->A));
  mix(g->arc_src.data(), g->arc_src.size() * 4);
  mix(g->arc_dst.data(), g->arc_dst.size() * 4);
  mix(g->arc_pdf.data(), g->arc_pdf.size() * 4);
  mix(g->arc_prob.data(), g->arc_prob.size() * 4);
  return h ? h : 1;
}

int64_t tc_chain_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T) {
  if (!g || S <= 0 || T <= 0) return TC_ERR_INVALID_ARGUMENT;
  return (int64_t)carve(nullptr, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g)).total;
}

int tc_den_forward_backward(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols,
                            int64_t y_stride, float leaky, float deriv_weight, float l2_scale, int accumulate,
                            float *deriv, int64_t deriv_stride, double *logprob_dev, int32_t *status_dev,
                            void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  if (!g || S <= 0 || rows <= 0 || rows % S != 0) return TC_ERR_INVALID_ARGUMENT;
  const int T = (int)(rows / S);
  Workspace w = carve((char *)workspace, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g));
  if (!workspace || (int64_t)w.total > workspace_bytes || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  DenParams p;
  int rc = fill_den_params(g, device, S, y, rows, cols, y_stride, leaky, deriv_weight, l2_scale, deriv, deriv_stride, w,
                           &p);
  if (rc != TC_OK) return rc;
  rc = launch_den_mode(p, accumulate, stream);
  if (rc != TC_OK) return rc;
  if (logprob_dev || status_dev)
    rc = launch_den_reduce(w.den_lp, deriv ? w.ab : nullptr, w.gs, S, logprob_dev, status_dev, stream);
  return rc;
}

int tc_den_forward_backward_ragged(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols,
                                   int64_t y_stride, float leaky, float deriv_weight, float l2_scale, int accumulate,
                                   float *deriv, int64_t deriv_stride, const int32_t *seq_frames_dev, int32_t max_frames,
                                   double *logprob_dev, int32_t *status_dev, void *workspace, int64_t workspace_bytes,
                                   int device, void *stream_v) {
  if (!g || S <= 0 || rows <= 0 || !seq_frames_dev || max_frames <= 0 || rows != (int64_t)max_frames * S)
    return TC_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)seq_frames_dev & 3) != 0) return TC_ERR_INVALID_ARGUMENT;
  if (g->big) return TC_ERR_UNSUPPORTED;  // (the streamed path: fill_den_params says why)
  const int T = max_frames;
  Workspace w = carve((char *)workspace, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g));
  if (!workspace || (int64_t)w.total > workspace_bytes || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  DenParams p;
  int rc = fill_den_params(g, device, S, y, rows, cols, y_stride, leaky, deriv_weight, l2_scale, deriv, deriv_stride, w,
                           &p, nullptr, seq_frames_dev);
  if (rc != TC_OK) return rc;
  rc = launch_den_mode(p, accumulate, stream);
  if (rc != TC_OK) return rc;
  // the kernels touch no padding row: written mode leaves +0 there, Kaldi's accumulating mode leaves them alone
  if (deriv && !accumulate)
    rc = launch_zero_padding(deriv, 4, deriv_stride, (int64_t)S * deriv_stride, 1, S, T, cols, seq_frames_dev, stream);
  if (rc != TC_OK) return rc;
  if (logprob_dev || status_dev)
    rc = launch_den_reduce(w.den_lp, deriv ? w.ab : nullptr, w.gs, S, logprob_dev, status_dev, stream);
  return rc;
}

int tc_num_forward_backward(tc_supervision *sup, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                            float *deriv, int64_t deriv_stride, double *logprob_dev, void *workspace,
                            int64_t workspace_bytes, int device, void *stream_v) {
  if (!sup) return TC_ERR_INVALID_ARGUMENT;
  const size_t need = align256((size_t)sup->S * 8);
  if (!workspace || (int64_t)need > workspace_bytes || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  NumParams p;
  int rc = fill_num_params(sup, device, stream, y, rows, cols, y_stride, deriv, deriv_stride, nullptr, 0,
                           (double *)workspace, &p);
  if (rc != TC_OK) return rc;
  rc = launch_num(p, stream);
  if (rc != TC_OK) return rc;
  if (logprob_dev) rc = launch_sum_double((const double *)workspace, sup->S, (double)sup->weight, logprob_dev, stream);
  if (rc != TC_OK) return rc;
  return supervision_mark_use(sup, device, stream);
}

int tc_supervision_best_path(tc_supervision *sup, const void *y, int dtype, int layout_bct, int64_t rows, int32_t cols,
                             int64_t y_stride, int32_t *pdf_dev, double *score_dev, int device, void *stream_v) {
  // (every argument check in front of the first device call)
  if (!sup || !y || !pdf_dev || !score_dev) return TC_ERR_INVALID_ARGUMENT;
  if (dtype != TC_DTYPE_F32 && dtype != TC_DTYPE_BF16 && dtype != TC_DTYPE_F16) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_bct && dtype != TC_DTYPE_F32) return TC_ERR_INVALID_ARGUMENT;  // (2-D tensors are float32, as NumParams::y)
  if ((int64_t)sup->S * sup->T != rows || sup->P != cols) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_bct && y_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  NumParams p;
  // (a (B, C, T) tensor has no row stride: fill_num_params is given the dense one)
  int rc = fill_num_params(sup, device, stream, (const float *)y, rows, cols, layout_bct ? (int64_t)cols : y_stride, nullptr,
                           0, nullptr, 0, nullptr, &p);
  if (rc != TC_OK) return rc;
  p.y_bct = layout_bct ? 1 : 0;
  p.elem = dtype;
  p.best_pdf = pdf_dev;
  p.best_score = score_dev;
  rc = launch_num_best_path(p, stream);
  if (rc != TC_OK) return rc;
  return supervision_mark_use(sup, device, stream);
}

int64_t tc_den_best_path_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T) {
  if (!g || S <= 0 || T <= 0) return TC_ERR_INVALID_ARGUMENT;
  return den_best_workspace_bytes(g->H, S, T);
}

int tc_den_best_path(tc_den_graph *g, int32_t S, const void *y, int dtype, int layout_bct, int64_t rows, int32_t cols,
                     int64_t y_stride, const int32_t *seq_frames_dev, int32_t max_frames, int32_t *pdf_dev,
                     int32_t *state_dev, double *score_dev, void *workspace, int64_t workspace_bytes, int device,
                     void *stream_v) {
  // (every argument check in front of the first device call)
  if (!g || !y || !pdf_dev || !score_dev || S <= 0 || max_frames <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (dtype != TC_DTYPE_F32 && dtype != TC_DTYPE_BF16 && dtype != TC_DTYPE_F16) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_bct && dtype != TC_DTYPE_F32) return TC_ERR_INVALID_ARGUMENT;  // (2-D tensors are float32)
  if (rows != (int64_t)S * max_frames || cols != g->P) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_bct && y_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)seq_frames_dev & 3) != 0) return TC_ERR_INVALID_ARGUMENT;
  if (!workspace || den_best_workspace_bytes(g->H, S, max_frames) > workspace_bytes || !aligned16(workspace))
    return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  DenBestParams p;
  const int rc = den_best_tables(g, device, &p.t);
  if (rc != TC_OK) return rc;
  p.y = (const float *)y;
  p.y_stride = layout_bct ? (int64_t)cols : y_stride;
  p.y_bct = layout_bct ? 1 : 0;
  p.elem = dtype;
  p.S = S;
  p.T = max_frames;
  p.H = g->H;
  p.P = g->P;
  p.Hs = (int)den_best_row_floats(g->H);
  p.seq_frames = seq_frames_dev;
  p.hist = (float *)workspace;
  p.pdf_out = pdf_dev;
  p.state_out = state_dev;
  p.score_out = score_dev;
  p.resident = den_best_resident(g->H) && !debug_flag(kDbgForceDenBestStreamed);
  return launch_den_best_path(p, (hipStream_t)stream_v);
}

int64_t tc_den_expected_accuracy_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T) {
  return tc_chain_workspace_bytes(g, S, T);
}

int64_t tc_den_expected_accuracy_grad_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T) {
  if (!g || S <= 0 || T <= 0) return TC_ERR_INVALID_ARGUMENT;
  return den_acc_grad_workspace_bytes(g->H, g->P, S, T);
}

// what the entries check alike, in front of any device call.  The hard pair: ref_dev, class_dev (nullable); the dense pair:
// accuracy, accuracy_stride (ref_dev and class_dev null).
static int den_accuracy_args(const tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                             const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const int32_t *ref_dev,
                             const int32_t *class_dev, const float *accuracy, int64_t accuracy_stride, bool dense,
                             const float *frame_acc_dev, const void *out, int64_t out_stride) {
  if (!g || !y || !(dense ? (const void *)accuracy : (const void *)ref_dev) || !frame_acc_dev || !out || S <= 0 || max_frames <= 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (rows != (int64_t)S * max_frames || cols != g->P || y_stride < cols || out_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (dense && accuracy_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (!(leaky >= 0.0f) || !(leaky <= FLT_MAX)) return TC_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)seq_frames_dev | (uintptr_t)ref_dev | (uintptr_t)class_dev | (uintptr_t)accuracy | (uintptr_t)frame_acc_dev |
        (uintptr_t)y) & 3) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  return TC_OK;
}

// tc_den_expected_accuracy and tc_den_expected_accuracy_dense
static int den_accuracy_value(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                              const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const int32_t *ref_dev,
                              const int32_t *class_dev, const float *accuracy, int64_t accuracy_stride, bool dense, float *gamma,
                              int64_t gamma_stride, float *frame_acc_dev, double *acc_dev, void *workspace,
                              int64_t workspace_bytes, int device, void *stream_v) {
  int rc = den_accuracy_args(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, ref_dev, class_dev, accuracy,
                             accuracy_stride, dense, frame_acc_dev, gamma, gamma_stride);
  if (rc != TC_OK) return rc;
  if (!acc_dev || ((uintptr_t)acc_dev & 7) != 0 || ((uintptr_t)gamma & 3) != 0) return TC_ERR_INVALID_ARGUMENT;
  if (!workspace || tc_chain_workspace_bytes(g, S, max_frames) > workspace_bytes || !aligned16(workspace))
    return TC_ERR_WORKSPACE;
  // the denominator posteriors, by whatever kernel the graph's class takes
  rc = seq_frames_dev ? tc_den_forward_backward_ragged(g, S, y, rows, cols, y_stride, leaky, 1.0f, 0.0f, 0, gamma, gamma_stride,
                                                       seq_frames_dev, max_frames, nullptr, nullptr, workspace,
                                                       workspace_bytes, device, stream_v)
                      : tc_den_forward_backward(g, S, y, rows, cols, y_stride, leaky, 1.0f, 0.0f, 0, gamma, gamma_stride,
                                                nullptr, nullptr, workspace, workspace_bytes, device, stream_v);
  if (rc != TC_OK) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  DenAccRowParams p;
  p.y = y;
  p.gamma = gamma;
  p.y_stride = y_stride;
  p.gamma_stride = gamma_stride;
  p.S = S;
  p.T = max_frames;
  p.P = g->P;
  p.seq_frames = seq_frames_dev;
  if (dense) {
    p.accuracy = accuracy;
    p.acc_stride = accuracy_stride;
  } else {
    p.ref = ref_dev;
    p.pdf_class = class_dev;
  }
  p.frame_acc = frame_acc_dev;
  p.acc = acc_dev;
  return launch_den_accuracy_rows(p, dense, (hipStream_t)stream_v);
}

// tc_den_expected_accuracy_grad and tc_den_expected_accuracy_dense_grad
static int den_accuracy_gradient(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                                 const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const int32_t *ref_dev,
                                 const int32_t *class_dev, const float *accuracy, int64_t accuracy_stride, bool dense,
                                 const float *frame_acc_dev, const float *seq_scale_dev, float *grad, int64_t grad_stride,
                                 void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  int rc = den_accuracy_args(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, ref_dev, class_dev, accuracy,
                             accuracy_stride, dense, frame_acc_dev, grad, grad_stride);
  if (rc != TC_OK) return rc;
  if ((((uintptr_t)grad | (uintptr_t)seq_scale_dev) & 3) != 0) return TC_ERR_INVALID_ARGUMENT;
  if (!workspace || den_acc_grad_workspace_bytes(g->H, g->P, S, max_frames) > workspace_bytes || !aligned16(workspace))
    return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  DenAccGradParams p;
  rc = den_acc_tables(g, device, &p.t);
  if (rc != TC_OK) return rc;
  p.y = y;
  p.y_stride = y_stride;
  p.S = S;
  p.T = max_frames;
  p.H = g->H;
  p.P = g->P;
  p.Hs = (int)den_acc_round4(g->H);
  p.Ps = (int)den_acc_round4(g->P);
  p.leaky = leaky;
  p.seq_frames = seq_frames_dev;
  if (dense) {
    p.accuracy = accuracy;
    p.acc_stride = accuracy_stride;
  } else {
    p.ref = ref_dev;
    p.pdf_class = class_dev;
  }
  p.frame_acc = frame_acc_dev;
  p.seq_scale = seq_scale_dev;
  p.grad = grad;
  p.grad_stride = grad_stride;
  p.workspace = (char *)workspace;
  p.resident = den_acc_resident(g->H, g->P) && !debug_flag(kDbgForceDenAccStreamed);
  return launch_den_accuracy_grad(p, dense, (hipStream_t)stream_v);
}

int tc_den_expected_accuracy(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                             const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const int32_t *ref_dev,
                             const int32_t *class_dev, float *gamma, int64_t gamma_stride, float *frame_acc_dev,
                             double *acc_dev, void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return den_accuracy_value(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, ref_dev, class_dev, nullptr, 0,
                            false, gamma, gamma_stride, frame_acc_dev, acc_dev, workspace, workspace_bytes, device, stream_v);
}

int tc_den_expected_accuracy_grad(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                                  const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const int32_t *ref_dev,
                                  const int32_t *class_dev, const float *frame_acc_dev, const float *seq_scale_dev,
                                  float *grad, int64_t grad_stride, void *workspace, int64_t workspace_bytes, int device,
                                  void *stream_v) {
  return den_accuracy_gradient(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, ref_dev, class_dev, nullptr, 0,
                               false, frame_acc_dev, seq_scale_dev, grad, grad_stride, workspace, workspace_bytes, device,
                               stream_v);
}

int tc_den_expected_accuracy_dense(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                                   const int32_t *seq_frames_dev, int32_t max_frames, float leaky, const float *accuracy,
                                   int64_t accuracy_stride, float *gamma, int64_t gamma_stride, float *frame_acc_dev,
                                   double *acc_dev, void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return den_accuracy_value(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, nullptr, nullptr, accuracy,
                            accuracy_stride, true, gamma, gamma_stride, frame_acc_dev, acc_dev, workspace, workspace_bytes,
                            device, stream_v);
}

int tc_den_expected_accuracy_dense_grad(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols,
                                        int64_t y_stride, const int32_t *seq_frames_dev, int32_t max_frames, float leaky,
                                        const float *accuracy, int64_t accuracy_stride, const float *frame_acc_dev,
                                        const float *seq_scale_dev, float *grad, int64_t grad_stride, void *workspace,
                                        int64_t workspace_bytes, int device, void *stream_v) {
  return den_accuracy_gradient(g, S, y, rows, cols, y_stride, seq_frames_dev, max_frames, leaky, nullptr, nullptr, accuracy,
                               accuracy_stride, true, frame_acc_dev, seq_scale_dev, grad, grad_stride, workspace,
                               workspace_bytes, device, stream_v);
}

int64_t tc_den_sample_paths_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T) {
  if (!g || S <= 0 || T <= 0) return TC_ERR_INVALID_ARGUMENT;
  return den_sample_workspace_bytes(g->H, S, T);
}

int tc_den_sample_paths(tc_den_graph *g, int32_t S, const float *y, int64_t rows, int32_t cols, int64_t y_stride,
                        const int32_t *seq_frames_dev, int32_t max_frames, float leaky, int32_t num_samples,
                        const float *uniforms_dev, int32_t *pdf_dev, int32_t *state_dev, void *workspace,
                        int64_t workspace_bytes, int device, void *stream_v) {
  // (every argument check in front of the first device call)
  if (!g || !y || !uniforms_dev || !pdf_dev || S <= 0 || max_frames <= 0 || num_samples <= 0) return TC_ERR_INVALID_ARGUMENT;
  if (rows != (int64_t)S * max_frames || cols != g->P || y_stride < cols) return TC_ERR_INVALID_ARGUMENT;
  if (!(leaky >= 0.0f) || !(leaky <= FLT_MAX)) return TC_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)y | (uintptr_t)seq_frames_dev | (uintptr_t)uniforms_dev | (uintptr_t)pdf_dev | (uintptr_t)state_dev) & 3) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (!workspace || den_sample_workspace_bytes(g->H, S, max_frames) > workspace_bytes || !aligned16(workspace))
    return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  DenSampleParams p;
  const int rc = den_acc_tables(g, device, &p.t);
  if (rc != TC_OK) return rc;
  p.y = y;
  p.y_stride = y_stride;
  p.S = S;
  p.T = max_frames;
  p.H = g->H;
  p.P = g->P;
  p.Hs = (int)den_acc_round4(g->H);
  p.K = num_samples;
  p.leaky = leaky;
  p.seq_frames = seq_frames_dev;
  p.uniforms = uniforms_dev;
  p.pdf_out = pdf_dev;
  p.state_out = state_dev;
  p.workspace = (char *)workspace;
  p.resident = den_sample_resident(g->H) && !debug_flag(kDbgForceDenSampleStreamed);
  return launch_den_sample_paths(p, (hipStream_t)stream_v);
}

int64_t tc_paths_edit_distance_workspace_bytes(int32_t S, int32_t K, int32_t max_frames) {
  if (S <= 0 || K <= 0 || max_frames <= 0) return TC_ERR_INVALID_ARGUMENT;
  return path_edit_workspace_bytes(S, K, max_frames);
}

int tc_paths_edit_distance(int32_t S, int32_t K, const int32_t *pdf_dev, const int32_t *seq_frames_dev, int32_t max_frames,
                           const int32_t *token_of_pdf_dev, const uint8_t *start_of_pdf_dev, int32_t P, const int32_t *ref_dev,
                           const int32_t *ref_len_dev, int32_t max_ref, int32_t *dist_dev, int32_t *len_dev,
                           int32_t *tokens_dev, void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  // (every argument check in front of the first device call)
  if (!pdf_dev || !token_of_pdf_dev || !dist_dev || !len_dev || S <= 0 || K <= 0 || max_frames <= 0 || P <= 0 || max_ref < 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (max_ref > 0 && (!ref_dev || !ref_len_dev)) return TC_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)pdf_dev | (uintptr_t)seq_frames_dev | (uintptr_t)token_of_pdf_dev | (uintptr_t)ref_dev |
        (uintptr_t)ref_len_dev | (uintptr_t)dist_dev | (uintptr_t)len_dev | (uintptr_t)tokens_dev) & 3) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (max_ref > kPathEditMaxRef || (int64_t)S * K > ((int64_t)1 << 31) - 1) return TC_ERR_UNSUPPORTED;
  if (!tokens_dev && (!workspace || path_edit_workspace_bytes(S, K, max_frames) > workspace_bytes || !aligned16(workspace)))
    return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  PathEditParams p;
  p.pdf = pdf_dev;
  p.seq_frames = seq_frames_dev;
  p.token_of_pdf = token_of_pdf_dev;
  p.start_of_pdf = start_of_pdf_dev;
  p.ref = ref_dev;
  p.ref_len = ref_len_dev;
  p.dist = dist_dev;
  p.len = len_dev;
  p.tokens = tokens_dev ? tokens_dev : (int32_t *)workspace;
  p.fill = tokens_dev ? 1 : 0;
  p.paths = (int64_t)S * K;
  p.K = K;
  p.T = max_frames;
  p.P = P;
  p.max_ref = max_ref;
  return launch_path_edit(p, (hipStream_t)stream_v);
}

int tc_sampled_risk_grad(int32_t S, int32_t K, int32_t max_frames, int32_t num_pdfs, const int32_t *pdf_dev,
                         const int32_t *seq_frames_dev, const double *weight_dev, const double *grad_output_dev,
                         const void *input, int dtype, int64_t input_stride_s, int64_t input_stride_c, int64_t input_stride_t,
                         void *grad, int64_t grad_stride_s, int64_t grad_stride_c, int64_t grad_stride_t, int64_t grad_elems,
                         int device, void *stream_v) {
  // (every argument check in front of the first device call)
  if (!pdf_dev || !weight_dev || !grad_output_dev || !input || !grad || S <= 0 || K <= 0 || max_frames <= 0 || num_pdfs <= 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (dtype != TC_DTYPE_F32 && dtype != TC_DTYPE_BF16 && dtype != TC_DTYPE_F16) return TC_ERR_INVALID_ARGUMENT;
  const int elem = dtype == TC_DTYPE_F32 ? 4 : 2;
  if (input_stride_s < 0 || input_stride_c < 0 || input_stride_t < 0 || grad_stride_s <= 0 || grad_stride_c <= 0 ||
      grad_stride_t <= 0)
    return TC_ERR_INVALID_ARGUMENT;
  // every element the kernel may store lies inside the block that is cleared
  if (grad_elems <= 0 || grad_elems > INT64_MAX / 4) return TC_ERR_INVALID_ARGUMENT;
  if ((__int128)(S - 1) * grad_stride_s + (__int128)(num_pdfs - 1) * grad_stride_c + (__int128)(max_frames - 1) * grad_stride_t >=
      (__int128)grad_elems)
    return TC_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)pdf_dev | (uintptr_t)seq_frames_dev) & 3) != 0 || (((uintptr_t)weight_dev | (uintptr_t)grad_output_dev) & 7) != 0 ||
      (((uintptr_t)input | (uintptr_t)grad) & (uintptr_t)(elem - 1)) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  if (K > kSampledRiskMaxSamples) return TC_ERR_UNSUPPORTED;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  TC_HIP_CHECK(hipMemsetAsync(grad, 0, (size_t)grad_elems * elem, stream));
  SampledRiskGradParams p;
  p.pdf = pdf_dev;
  p.seq_frames = seq_frames_dev;
  p.weight = weight_dev;
  p.grad_out = grad_output_dev;
  p.input = input;
  p.grad = grad;
  p.in_s = input_stride_s;
  p.in_c = input_stride_c;
  p.in_t = input_stride_t;
  p.g_s = grad_stride_s;
  p.g_c = grad_stride_c;
  p.g_t = grad_stride_t;
  p.S = S;
  p.K = K;
  p.T = max_frames;
  p.C = num_pdfs;
  return launch_sampled_risk_grad(p, dtype, stream);
}

}  // extern "C"

// deriv_scale = 1: the reference's outputs.  deriv_scale = -1: what its backward returns (tc_chain_objf_and_grad).
// bct_input (tc_chain_step, (B, C, T) tensors): `y` is scratch that this call fills from bct_input (tc_to2d) in front of the
// denominator; the numerator, which reads y at the supervision's (frame, pdf) pairs only, reads bct_input where it lies
// and runs BESIDE that copy and the denominator on the side stream (its posteriors wait in the supervision's staging
// area for the scatter behind the denominator, as for small batches).
// xent_out / xent_objf_dev (tc_chain_step): the cross-entropy output and where sum(xent_out * xent) goes -- formed from
// the numerator's posteriors as they are written, not from the dense matrices
// xent_row_w (tc_chain_step_weighted): the per-row factor of the xent entries the numerator writes (not of its objective sum)
struct ObjfStep {  // what only the one-call step passes: all unset for the two plain entry points
  const float *xent_out = nullptr, *bct_input = nullptr, *xent_row_w = nullptr;
  int64_t xent_out_stride = 0;
  double *xent_objf_dev = nullptr;
  float *loss_dev1 = nullptr;
  int xent_bct = 0, xent_out_bct = 0, bct_dtype = TC_DTYPE_F32;
  bool xent_sums_ready = false;  // (the numerator-only pass of kaldi_way == 0 has left the sequences' xent sums)
  // the step moves deriv / xent on (emit_gradients) and zeroes a ragged minibatch's padding in the caller's tensors itself
  bool outputs_move_on = false;
  // tc_chain_step_per_sequence: the sequences' own values ([S][6] doubles, nullable) and whether a failed sequence is masked
  // out of the sums; either one selects the per-sequence finalize (alive_frames is then written to the workspace)
  double *seq_results = nullptr;
  bool isolate = false;
  // tc_chain_step_log_softmax: the row statistics of xent_out ([rows][2], launch_xent_row_stats); the numerator's
  // cross-entropy sums are then taken on the rows' log-softmax (NumParams::xent_lse)
  const float *xent_lse = nullptr;
  // tc_chain_step_boosted: `y` is the denominator's private matrix y_b, scratch that this call fills in front of the
  // denominator (boost_kernels.hip) from bct_input, or from the rows of boost_src (unit channel stride, element (s, c, t) at
  // s * boost_sb + t * boost_st, of bct_dtype).  The numerator reads the true y: bct_input where it lies, else num_y.  The l2
  // term is put back on the true y behind the denominator (the sequences' sums) and behind the soft-failure reset (deriv).
  const BoostAcc *boost = nullptr;
  const void *boost_src = nullptr;
  int64_t boost_sb = 0, boost_st = 0;
  const float *num_y = nullptr;
  int64_t num_y_stride = 0;
};

static int chain_objf(tc_den_graph *g, tc_supervision *sup, const float *y, int64_t rows, int32_t cols,
                      int64_t y_stride, float *results_dev3, float *deriv, int64_t deriv_stride, float *xent,
                      int64_t xent_stride, float l2_regularize, float leaky, float deriv_scale, float xent_scale,
                      void *workspace, int64_t workspace_bytes, int device, void *stream_v, const ObjfStep &o = ObjfStep()) {
  if (!g || !sup || !y || !results_dev3) return TC_ERR_INVALID_ARGUMENT;
  if (sup->P != g->P) return TC_ERR_INVALID_ARGUMENT;
  if ((int64_t)sup->S * sup->T != rows) return TC_ERR_INVALID_ARGUMENT;
  Workspace w = carve((char *)workspace, hist_states(g), sup->S, sup->T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, sup->S), pair_room(g), planes_room(g));
  if (!workspace || (int64_t)w.total > workspace_bytes || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;

  const float wgt = sup->weight;
  DenParams dp;
  // (deriv_scale is +-1: the products below are exact, so the scaled outputs are the exact negatives)
  int rc = fill_den_params(g, device, sup->S, y, rows, cols, y_stride, leaky, deriv_scale * -wgt,
                           deriv_scale * (wgt * l2_regularize), deriv, deriv_stride, w, &dp);
  if (rc != TC_OK) return rc;
  // A ragged supervision: its lengths, in the pool slot with its tables, are the denominator's loop bounds too (the
  // numerator's upload below is enqueued on this stream in front of both).  The kernels touch no padding row.
  const bool ragged = !sup->frames.empty();
  if (ragged && g->big) return TC_ERR_UNSUPPORTED;
  NumParams np;
  rc = fill_num_params(sup, device, stream, y, rows, cols, y_stride, deriv, deriv_stride, xent, xent_stride, w.num_lp,
                       &np);
  if (rc != TC_OK) return rc;
  np.deriv_scale = deriv_scale;
  np.xent_scale = xent_scale;
  if (o.boost && o.num_y) {
    np.y = o.num_y;
    np.y_stride = o.num_y_stride;
  }
  BoostAcc boost;
  if (o.boost) {
    boost = *o.boost;
    boost.seq_frames = ragged ? np.seq_frames : nullptr;
  }
  if (ragged) {
    dp.set_seq_frames(np.seq_frames);
    count_launch(kCntRagged);
  }
  if (o.xent_out && o.xent_objf_dev) {  // (also without the dense xent matrix: an evaluation step's cross-entropy objective)
    np.xent_out = o.xent_out;
    np.xent_out_stride = o.xent_out_stride;
    np.xent_out_bct = o.xent_out_bct;
    np.seq_xent = w.xent_lp;
    np.xent_lse = o.xent_lse;
  }
  np.xent_bct = o.xent_bct;  // (a (B, C, T) tensor the caller has cleared: only the posteriors' entries are written)
  np.xent_row_w = xent ? o.xent_row_w : nullptr;  // (tc_chain_step_weighted: the numerator is xent's only non-zero writer)
  if (o.bct_input) {
    np.y = o.bct_input;
    np.y_bct = 1;
    np.elem = o.bct_dtype;  // (bct_input and a (B, C, T) xent_out: the caller's tensors, float32 or 16-bit)
  }
  auto fill_y = [&]() -> int {  // the frame-major copy the denominator reads
    if (o.boost && o.bct_input)
      return launch_boost_bct(o.bct_dtype, o.bct_input, const_cast<float *>(y), y_stride, sup->S, cols, sup->T, boost, stream);
    if (o.boost)
      return launch_boost_rows(o.bct_dtype, o.boost_src, o.boost_sb, o.boost_st, const_cast<float *>(y), y_stride, sup->S, sup->T,
                               cols, boost, stream);
    return o.bct_input ? launch_to2d(o.bct_dtype, o.bct_input, const_cast<float *>(y), sup->S, cols, sup->T, y_stride, stream) : TC_OK;
  };

  SideStreams *ss = nullptr;
  rc = side_streams(stream, &ss);
  if (rc != TC_OK) return rc;
  if (xent && !o.xent_bct) {
    // xent_deriv is zero outside the numerator's posteriors.  The denominator kernels that write every row of deriv
    // anyway write these zero rows with them (under their arc walks, where stores cost next to nothing); the others get
    // a memset in front: 629 MB at C3, 0.13 ms.
    if (deriv && den_zeroes_xent(dp, ss->num_cus)) {
      dp.xent_zero = xent;
      dp.xent_stride = xent_stride;
      dp.x_vec = (cols % 4 == 0 && xent_stride % 4 == 0 && aligned16(xent)) ? 1 : 0;
    } else if (xent_stride == cols) {
      TC_HIP_CHECK(hipMemsetAsync(xent, 0, (size_t)rows * cols * sizeof(float), stream));
    } else {
      TC_HIP_CHECK(hipMemset2DAsync(xent, (size_t)xent_stride * 4, 0, (size_t)cols * 4, (size_t)rows, stream));
    }
  }
  // denominator first: it writes every element of deriv (-w*gamma_den - w*l2*y); the numerator then
  // adds its sparse posteriors.  [K] runs the numerator first; the sum is the same.
  // When the denominator leaves CUs idle (small batches) the numerator's recursion runs beside it on a side
  // stream, leaving its posteriors in the supervision's staging area; the scatter follows the denominator.
  // (a forward-only call overlaps the two forward recursions the same way; its numerator writes nothing but its sums)
  if ((o.bct_input || den_cus_used(dp, ss->num_cus) + 16 <= ss->num_cus) && np.t.stage && !debug_flag(kDbgNoNumOverlap)) {
    std::lock_guard<std::recursive_mutex> lock(ss->enqueue);
    np.staged = 1;
    TC_HIP_CHECK(hipEventRecord(ss->num_fork, stream));
    TC_HIP_CHECK(hipStreamWaitEvent(ss->num_side, ss->num_fork, 0));
    rc = launch_num(np, ss->num_side);
    if (rc == TC_OK) rc = fill_y();
    if (rc == TC_OK) rc = launch_den(dp, stream);
    // Join the side stream also when something failed after the fork: the caller sees an error and may free or reuse
    // the workspace and the supervision, which the numerator kernel could still be reading or writing -- and the
    // supervision's pool slot must learn of its last reader before it can be handed out again.
    hipError_t e = hipEventRecord(ss->num_join, ss->num_side);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, ss->num_join, 0);
    if (rc != TC_OK || e != hipSuccess) {
      (void)supervision_mark_use(sup, device, stream);
      if (rc != TC_OK) return rc;
      TC_HIP_CHECK(e);
    }
    rc = launch_num_scatter(np, stream);
    if (rc != TC_OK) {
      (void)supervision_mark_use(sup, device, stream);
      return rc;
    }
  } else {
    rc = fill_y();
    if (rc == TC_OK) rc = launch_den(dp, stream);
    if (rc != TC_OK) return rc;
    rc = launch_num(np, stream);
    if (rc != TC_OK) return rc;
  }
  rc = supervision_mark_use(sup, device, stream);
  if (rc != TC_OK) return rc;
  // (the boosted step: the denominator summed y_b^2; the l2 term is the true y's)
  if (o.boost && l2_regularize != 0.0f) {
    rc = launch_boost_l2_sum(y, y_stride, sup->S, sup->T, cols, boost, w.y2, stream);
    if (rc != TC_OK) return rc;
  }
  const double *xent_sums = (np.seq_xent || o.xent_sums_ready) && o.xent_objf_dev ? w.xent_lp : nullptr;
  if (o.isolate || o.seq_results)
    rc = launch_finalize_per_sequence(w.den_lp, w.num_lp, w.y2, w.ab, w.gs, sup->S, sup->T, wgt, l2_regularize, deriv != nullptr,
                                      results_dev3, w.fail, stream, xent_sums, o.xent_objf_dev, o.loss_dev1,
                                      ragged ? sup->total_frames : 0, ragged ? np.seq_frames : nullptr, o.isolate ? 1 : 0,
                                      o.seq_results, w.alive_frames);
  else
    rc = launch_finalize(w.den_lp, w.num_lp, w.y2, w.ab, w.gs, sup->S, sup->T, wgt, l2_regularize, deriv != nullptr,
                         results_dev3, w.fail, stream, xent_sums, o.xent_objf_dev, o.loss_dev1, ragged ? sup->total_frames : 0);
  if (rc != TC_OK) return rc;
  // (a (B, C, T) xent tensor is rows * cols contiguous floats: cleared as such)
  rc = launch_zero_on_fail(w.fail, deriv, deriv_stride, xent, o.xent_bct ? (int64_t)cols : xent_stride, y, y_stride,
                           deriv_scale * (wgt * l2_regularize), rows, cols, stream);
  // (the boosted step: the denominator, and the reset just now, wrote -l2_scale * y_b)
  if (rc == TC_OK && o.boost && deriv && l2_regularize != 0.0f)
    rc = launch_boost_l2_grad(deriv, deriv_stride, sup->S, sup->T, cols, boost, deriv_scale * (wgt * l2_regularize), stream);
  // ragged: +0 in the padding rows, which no kernel wrote (and the failure route just filled from y's padding)
  if (rc == TC_OK && ragged && !o.outputs_move_on) {
    if (deriv) rc = launch_zero_padding(deriv, 4, deriv_stride, (int64_t)sup->S * deriv_stride, 1, sup->S, sup->T, cols, np.seq_frames, stream);
    if (rc == TC_OK && xent) rc = launch_zero_padding(xent, 4, xent_stride, (int64_t)sup->S * xent_stride, 1, sup->S, sup->T, cols, np.seq_frames, stream);
  }
  return rc;
}

extern "C" {

int tc_chain_objf_and_deriv(tc_den_graph *g, tc_supervision *sup, const float *y, int64_t rows, int32_t cols,
                            int64_t y_stride, float *results_dev3, float *deriv, int64_t deriv_stride, float *xent,
                            int64_t xent_stride, float l2_regularize, float leaky, float xent_regularize,
                            void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  (void)xent_regularize;  // as in the reference it only decides whether the caller passes xent (my_lib_chain.cpp:127)
  return chain_objf(g, sup, y, rows, cols, y_stride, results_dev3, deriv, deriv_stride, xent, xent_stride, l2_regularize,
                    leaky, 1.0f, 1.0f, workspace, workspace_bytes, device, stream_v);
}

int tc_chain_objf_and_grad(tc_den_graph *g, tc_supervision *sup, const float *y, int64_t rows, int32_t cols,
                           int64_t y_stride, float *results_dev3, float *grad, int64_t grad_stride, float *xent_grad,
                           int64_t xent_stride, float l2_regularize, float leaky, float xent_regularize,
                           void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return chain_objf(g, sup, y, rows, cols, y_stride, results_dev3, grad, grad_stride, xent_grad, xent_stride,
                    l2_regularize, leaky, -1.0f, -xent_regularize, workspace, workspace_bytes, device, stream_v);
}

// ---- one call per training step --------------------------------------------------------------------------------
// Workspace of tc_chain_step: [tc_chain_workspace_bytes | scratch of the xent objective | for (B, C, T) tensors the
// frame-major copies of input and gradient (and of xent_input and its gradient)].  16-bit tensors (tc_chain_step_typed):
// the float32 copies of input and gradient (and xent_input) in 2-D as well, then the float32 xent gradient.
namespace {
struct StepWorkspace {
  char *chain, *trace;
  float *y2d, *g2d, *x2d, *xg;
  float *lse;  // tc_chain_step_log_softmax: xent_input's row statistics, [S * T][2] (behind everything the siblings carve)
  float *yb;   // tc_chain_step_boosted: the denominator's matrix where y2d holds (or the caller's tensor is) the true y
  size_t chain_bytes, total;
};
StepWorkspace carve_step(char *base, const tc_den_graph *g, int S, int T, int P, bool three_d, bool xent,
                         int dtype = TC_DTYPE_F32, bool log_softmax = false, bool boosted_rows = false) {
  StepWorkspace w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  w.chain_bytes = carve(nullptr, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g)).total;
  w.chain = take(w.chain_bytes);
  w.trace = take((size_t)trace_workspace_bytes());
  const size_t mat = (size_t)S * T * P * sizeof(float);
  const bool half = dtype != TC_DTYPE_F32, copies = three_d || half;
  w.y2d = copies ? (float *)take(mat) : nullptr;
  w.g2d = copies ? (float *)take(mat) : nullptr;
  w.x2d = copies && xent ? (float *)take(mat) : nullptr;
  w.xg = half && xent ? (float *)take(mat) : nullptr;
  w.lse = log_softmax && xent ? (float *)take((size_t)S * T * 2 * sizeof(float)) : nullptr;
  w.yb = boosted_rows ? (float *)take(mat) : nullptr;
  w.total = off;
  return w;
}
}  // namespace

static bool known_dtype(int dtype) { return dtype == TC_DTYPE_F32 || dtype == TC_DTYPE_BF16 || dtype == TC_DTYPE_F16; }

int64_t tc_chain_step_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T, int three_d, int with_xent) {
  return tc_chain_step_typed_workspace_bytes(g, S, T, three_d, with_xent, TC_DTYPE_F32);
}

int64_t tc_chain_step_typed_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T, int three_d, int with_xent,
                                            int dtype) {
  if (!g || S <= 0 || T <= 0 || !known_dtype(dtype)) return TC_ERR_INVALID_ARGUMENT;
  return (int64_t)carve_step(nullptr, g, S, T, g->P, three_d != 0, with_xent != 0, dtype).total;
}

// The step in every layout (TC_LAYOUT_*), in three stages: the way in (gather / widen / clear), the objective (the
// numerator-only pass of kaldi_way == 0, then chain_objf), and emit_gradients, the last pass over each gradient.  StepIo is
// what the stages share.  batch_stride / frame_stride (sb, st): TC_LAYOUT_CHANNEL_LAST only, checked by the caller.
// Between the way in and the way out runs the float32 frame-major step: on float32 2-D tensors as they are, on 16-bit 2-D
// tensors widened and channel-last views gathered (launch_rows_gather) into contiguous float32 scratch, on (B, C, T) tensors
// copied into it inside chain_objf, beside the numerator, which reads them where they lie.  The last pass -- the (B, C, T)
// copy back, the rounding pass, the channel-last scatter -- applies row weight, penalty and the one rounding behind
// chain_objf's soft-failure reset.  A channel-last step's 2-D xent gradient needs one more float32 matrix than the (B, C, T)
// step has: for 16-bit tensors the float32 xent scratch that step has anyway; for float32 the caller's `grad`, which has
// exactly that size and is written last, by the MMI gradient's scatter.
namespace {
struct StepIo {
  const float *y, *bct_input;     // the frame-major matrix the objective reads; the (B, C, T) tensor chain_objf fills it from
  float *gr, *xg;                 // what the objective writes, P floats a row: MMI and xent gradient (NULL: not wanted)
  const float *num_in, *xent_in;  // kaldi_way == 0's numerator-only pass reads num_in; the xent objective is formed with xent_in
  int64_t y_stride, num_stride, xent_stride;
  int caller_bct, xent_bct;       // num_in / xent_in are the caller's (B, C, T) tensors; xg is a cleared (B, C, T) gradient
};

// The table.  scratch: the objective runs on the workspace's float32 copies (every case but float32 2-D).  widened: so do
// the numerator's reads of the network outputs (16-bit 2-D and channel-last; a (B, C, T) tensor is read where it lies).
// second_only (kaldi_way == 0 with the regulariser): the one objective call is made on xent_input.
StepIo step_io(const StepWorkspace &w, int layout, bool half, bool eval_only, bool second_only, bool use_xent, int P,
               int64_t row_stride, const float *input, const float *xent_input, float *grad, float *xent_grad) {
  const bool cl = layout == TC_LAYOUT_CHANNEL_LAST, bct = layout == TC_LAYOUT_BCT;
  const bool scratch = layout != TC_LAYOUT_ROWS || half, widened = cl || (half && !bct);
  StepIo io;
  io.y = scratch ? (second_only ? w.x2d : w.y2d) : (second_only ? xent_input : input);
  io.y_stride = scratch ? (int64_t)P : row_stride;
  io.gr = eval_only ? nullptr : (scratch ? w.g2d : grad);
  // (16-bit: float32 scratch, rounded at the end; float32 channel-last: the caller's grad, until its scatter fills it)
  io.xg = !use_xent || eval_only ? nullptr : (half ? w.xg : (cl ? grad : xent_grad));
  io.num_in = widened ? w.y2d : input;
  io.num_stride = widened || bct ? (int64_t)P : row_stride;
  io.xent_in = widened ? w.x2d : xent_input;
  io.xent_stride = widened ? (int64_t)P : row_stride;
  io.bct_input = bct ? (second_only ? xent_input : input) : nullptr;
  io.caller_bct = bct ? 1 : 0;
  // (xent_deriv has entries only where the numerator has posteriors: written straight into the cleared (B, C, T) gradient)
  io.xent_bct = bct && use_xent ? 1 : 0;
  return io;
}

// The last pass over each gradient, picked from (layout, dtype, penalty, weights): the MMI gradient becomes w[row] * (g + t),
// (-1 * w[row]) * g in one multiply where the sign is still to come, rounded once for 16-bit tensors.  The xent gradient is
// final as the numerator left it (scaled and weighted): it is only moved or rounded.
int emit_gradients(const StepIo &io, int layout, int dtype, const float *input, int64_t row_stride, int64_t sb, int64_t st,
                   float *grad, float *xent_grad, const float *y2d, int S, int T, int P, float pen_c2, const float *row_w,
                   int device, void *stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const bool half = dtype != TC_DTYPE_F32, cl = layout == TC_LAYOUT_CHANNEL_LAST, bct = layout == TC_LAYOUT_BCT;
  const int64_t rows = (int64_t)S * T;
  // 3-D: the sign is still to come.  y where the pass's output lies: the caller's tensor, or its widened copy (16-bit 2-D)
  LastPass lp;
  lp.scale = cl || bct ? -1.0f : 1.0f;
  lp.row_w = row_w;
  lp.pen_c2 = pen_c2;
  lp.y = !cl && !bct && half ? y2d : input;
  lp.y_stride = cl ? sb : row_stride;
  lp.y_st = st;
  int rc = TC_OK;
  if (cl) {
    // dense (B, T, C) gradients; the xent gradient first: for float32 it lies in `grad`
    const int64_t dense_b = (int64_t)T * P;
    LastPass moved;
    moved.scaled = false;
    if (io.xg) rc = launch_rows_scatter(dtype, io.xg, P, xent_grad, dense_b, P, S, T, P, moved, stream);
    if (rc == TC_OK) rc = launch_rows_scatter(dtype, io.gr, P, grad, dense_b, P, S, T, P, lp, stream);
    return rc;
  }
  if (bct) {
    // (plain float32: tc_from2d itself, whose limits the other cases were held to with the arguments)
    if (half || row_w || pen_c2 > 0.0f) rc = launch_from2d(dtype, io.gr, P, grad, S, P, T, lp, stream);
    else rc = tc_from2d(io.gr, P, S, P, T, lp.scale, grad, device, stream_v);
  } else if (half) {
    // the one rounding of every element, from the float32 values tc_chain_step would have returned
    rc = launch_round(dtype, io.gr, grad, rows * P, P, lp, stream);
  } else if (row_w || pen_c2 > 0.0f) {
    // float32 2-D: the denominator and the numerator have written the caller's tensor; one pass in place, behind
    // chain_objf's launch_zero_on_fail, so a soft failure's -l2 * weight * y is penalised and weighted too
    rc = launch_scale_rows(io.gr, rows, P, lp, stream);
  }
  if (rc == TC_OK && half && io.xg) rc = launch_round(dtype, io.xg, xent_grad, rows * P, P, LastPass{}, stream);
  return rc;
}
}  // namespace

static int chain_step_layout(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int layout,
                             int64_t row_stride, int64_t sb, int64_t st, float l2_regularize, float leaky,
                             float xent_regularize, int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3,
                             float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                             float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                             void *stream_v, int isolate_failures = 0, double *seq_results_dev = nullptr,
                             int xent_log_softmax = 0, const BoostAcc *boost = nullptr) {
  if (!g || !sup || !input_v || !results_dev3 || !known_dtype(dtype)) return TC_ERR_INVALID_ARGUMENT;
  // (with kaldi_way == 0 the whole objective is run again on xent_input: what a log-softmax in front of that means is
  // another question)
  if (xent_log_softmax && !kaldi_way) return TC_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)seq_results_dev & 7) != 0) return TC_ERR_INVALID_ARGUMENT;
  // (the boosted step with kaldi_way == 0 and the xent branch: which of the two objective calls is boosted is another question)
  if (boost && !kaldi_way && xent_input_v != nullptr && xent_regularize != 0.0f) return TC_ERR_INVALID_ARGUMENT;
  const bool cl = layout == TC_LAYOUT_CHANNEL_LAST;
  const int three_d = layout != TC_LAYOUT_ROWS;
  if (((uintptr_t)deriv_weights & 3) != 0) return TC_ERR_INVALID_ARGUMENT;
  if (!(out_of_range_regularize >= 0.0f) || std::isinf(out_of_range_regularize)) return TC_ERR_INVALID_ARGUMENT;
  // (16-bit tensors travel as float pointers up to the kernels that read or write them: NumParams::elem, launch_to2d)
  const float *input = static_cast<const float *>(input_v), *xent_input = static_cast<const float *>(xent_input_v);
  float *grad = static_cast<float *>(grad_v), *xent_grad = static_cast<float *>(xent_grad_v);
  const bool half = dtype != TC_DTYPE_F32;
  const bool use_xent = xent_input != nullptr && xent_regularize != 0.0f;
  // grad == NULL: an evaluation step ([K] ComputeChainObjfAndDeriv with nnet_output_deriv == NULL, as Kaldi's own
  // diagnostics call it): the two forward recursions, the results and the loss; no Backward(), so no alpha-beta
  // check, no gradient written, no copy back.  (The reference's validation loop pays for a whole training step under
  // torch.no_grad(): example/chime5/train.py:150-171 -> torchain/functions.py:74,82 allocate and fill mmi_grad anyway.)
  const bool eval_only = grad == nullptr;
  if (eval_only && xent_grad) return TC_ERR_INVALID_ARGUMENT;
  if (!eval_only && use_xent && !xent_grad) return TC_ERR_INVALID_ARGUMENT;
  const int S = sup->S, T = sup->T, P = sup->P;
  if (P != g->P) return TC_ERR_INVALID_ARGUMENT;
  const int64_t rows = (int64_t)S * T;
  if (!three_d && row_stride < P) return TC_ERR_INVALID_ARGUMENT;
  // (tc_from2d's limits; the float32 unweighted call meets them in tc_from2d itself)
  if ((half || deriv_weights || out_of_range_regularize > 0.0f) && three_d && !cl && !layout_grid_ok(S, T))
    return TC_ERR_UNSUPPORTED;
  // Kaldi's deriv_weights ([K] nnet-chain-training.cc: MulRowsVec on both derivatives, after the objectives are formed):
  // ignored by an evaluation step, which writes no gradient.  Every gradient element becomes w[row] * g, one float32
  // multiply of the unweighted value, in whichever pass writes it last (emit_gradients; the numerator's stores for xent).
  const float *row_w = eval_only ? nullptr : deriv_weights;
  // The out-of-range penalty (after [K] PenalizeOutOfRange, restated in torchain_hip.h): t = fl32(2c) * p(y) joins the
  // MMI gradient in the same last passes, in front of the row weight; y is always the chain output `input`, also when
  // kaldi_way == 0 runs the objective on xent_input.  pen_c2 == 0: none of this runs.
  const float pen_c2 = eval_only ? 0.0f : 2.0f * out_of_range_regularize;
  if (std::isinf(pen_c2)) return TC_ERR_INVALID_ARGUMENT;
  // Kaldi's log-softmax at the end of the cross-entropy head, folded in (xent_softmax_kernels.hip): without the xent branch
  // the option does nothing
  const bool lsm = xent_log_softmax != 0 && use_xent;
  // (the boosted step's own matrix: a (B, C, T) step has y2d free for it; every other layout keeps the true y there or reads
  // it in the caller's tensor.  Its workspace is sized with the row statistics whether the switch is on or not.)
  const bool boosted_rows = boost != nullptr && layout != TC_LAYOUT_BCT;
  const StepWorkspace w = carve_step((char *)workspace, g, S, T, P, three_d != 0, use_xent, dtype, lsm || boost != nullptr, boosted_rows);
  if (!workspace || (int64_t)w.total > workspace_bytes || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  if (cl && !channel_last_strides_ok(S, T, P, sb, st)) return TC_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  hipStream_t stream = (hipStream_t)stream_v;
  // The reference's way (kaldi_way == 0, functions.py:96-103) makes a second objective call on xent_input INTO THE SAME
  // results, gradient and xent gradient: everything the first call wrote is overwritten.  Only that second call is made
  // here; what remains of the first is this library's own extra, the cross-entropy objective, which is defined on the
  // first call's xent_deriv: the numerator alone on `input` (no denominator, nothing written but the sequences' sums).
  const bool second_only = use_xent && !kaldi_way;
  StepIo io = step_io(w, layout, half, eval_only, second_only, use_xent, P, row_stride, input, xent_input, grad, xent_grad);
  if (boosted_rows) {  // the denominator's matrix; the numerator keeps io.num_in
    io.y = w.yb;
    io.y_stride = P;
  }
  int rc = TC_OK;

  // ---- the way in
  if (cl) {
    // (the chain output's rows are read by the objective, or with kaldi_way == 0 by the numerator-only pass alone)
    if (!second_only || xent_objf_dev) rc = launch_rows_gather(dtype, input, sb, st, w.y2d, P, S, T, P, stream);
    if (rc == TC_OK && use_xent) rc = launch_rows_gather(dtype, xent_input, sb, st, w.x2d, P, S, T, P, stream);
    if (rc != TC_OK) return rc;
    count_launch(kCntChannelLast);
  } else if (three_d) {
    if (io.xg) TC_HIP_CHECK(hipMemsetAsync(io.xg, 0, (size_t)rows * P * sizeof(float), stream));
  } else if (half) {
    rc = launch_widen_rows(dtype, input, row_stride, w.y2d, rows, P, stream);
    if (rc == TC_OK && use_xent) rc = launch_widen_rows(dtype, xent_input, row_stride, w.x2d, rows, P, stream);
    if (rc != TC_OK) return rc;
  }
  // (the rows of xent_input where the objective finds them: an evaluation step without xent_objf_dev has no use for them)
  if (lsm && (xent_objf_dev || !eval_only)) {
    rc = launch_xent_row_stats(io.caller_bct ? dtype : TC_DTYPE_F32, io.xent_in, io.caller_bct, io.xent_stride, S, T, P, w.lse,
                               stream);
    if (rc != TC_OK) return rc;
  }

  // ---- the objective
  // 2-D: the matrices leave as the reference's backward returns them (-deriv, -xent_regularize * xent_deriv); 3-D: the
  // MMI gradient's sign rides on the way back (copy back or scatter), so the 2-D scratch holds the plain derivative
  const float dscale = three_d ? 1.0f : -1.0f, xscale = -xent_regularize;  // (the xent gradient: final values everywhere)
  // Kaldi's cross-entropy objective sum(xent_output * xent_deriv) ([K] nnet-chain-training.cc; a TODO in the reference,
  // torchain/functions.py:88-89): xent_objf_dev receives it times `xscale`, summed by the numerator over the entries it
  // writes (tc_xent_objf is the dense statement of the same sum)
  if (second_only && xent_objf_dev) {
    const Workspace wi = carve((char *)w.chain, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g));
    NumParams np;
    rc = fill_num_params(sup, device, stream, io.num_in, rows, P, io.num_stride, nullptr, 0, nullptr, 0, wi.num_lp, &np);
    if (rc != TC_OK) return rc;
    np.y_bct = io.caller_bct;
    np.elem = io.caller_bct ? dtype : TC_DTYPE_F32;
    np.xent_scale = xscale;
    np.xent_out = io.xent_in;
    np.xent_out_stride = io.xent_stride;
    np.xent_out_bct = io.caller_bct;
    np.seq_xent = wi.xent_lp;
    rc = launch_num(np, stream);
    if (rc == TC_OK) rc = supervision_mark_use(sup, device, stream);
    if (rc != TC_OK) return rc;
  }
  ObjfStep o;
  o.xent_out = use_xent && !second_only ? io.xent_in : nullptr;
  o.xent_out_stride = io.xent_stride;
  o.xent_objf_dev = use_xent ? xent_objf_dev : nullptr;
  o.xent_bct = o.xent_out_bct = io.xent_bct;
  o.bct_input = io.bct_input;
  o.xent_sums_ready = second_only && xent_objf_dev != nullptr;
  o.loss_dev1 = loss_dev1;  // (the loss value -objf / weight is written with the results: finalize_kernel)
  o.bct_dtype = dtype;
  o.xent_row_w = row_w;
  o.outputs_move_on = true;
  o.isolate = isolate_failures != 0;
  o.seq_results = seq_results_dev;
  o.xent_lse = lsm ? w.lse : nullptr;
  if (boost) {
    o.boost = boost;
    if (boosted_rows) {
      o.boost_src = input;
      o.boost_sb = cl ? sb : row_stride;
      o.boost_st = cl ? st : (int64_t)S * row_stride;
      o.num_y = io.num_in;
      o.num_y_stride = io.num_stride;
    }
  }
  rc = chain_objf(g, sup, io.y, rows, P, io.y_stride, results_dev3, io.gr, P, io.xg, P, l2_regularize, leaky, dscale, xscale,
                  w.chain, (int64_t)w.chain_bytes, device, stream_v, o);
  if (rc != TC_OK || eval_only) return rc;
  const bool ragged = !sup->frames.empty();
  const int32_t *frames_dev = nullptr, *alive = nullptr;
  if (ragged) {
    std::lock_guard<std::mutex> lock(sup->mu);
    frames_dev = sup->frames_dev[device];
  }
  // (the isolating step: every sequence's surviving frames, left in the workspace by the finalize -- see below)
  if (o.isolate)
    alive = carve((char *)w.chain, hist_states(g), S, T, big_p(g), big_h(g), big_g(g), big_hb(g), split_room(g, S), pair_room(g), planes_room(g)).alive_frames;
  // ---- the log-softmax's backward: the xent gradient V, final but for its move or rounding, becomes V - rowsum(V) *
  // softmax(xent_input) in the float32 matrix the numerator wrote it to.  Behind chain_objf's soft-failure reset (rows of no
  // mass become +0), over the rows the tail below does not zero: a sequence's own frames, none of a failed sequence.
  if (lsm) {
    rc = launch_xent_softmax_grad(io.caller_bct ? dtype : TC_DTYPE_F32, io.xent_in, io.caller_bct, io.xent_stride, io.xg, P, S, T,
                                  P, w.lse, o.isolate ? alive : frames_dev, stream);
    if (rc != TC_OK) return rc;
  }
  rc = emit_gradients(io, layout, dtype, input, row_stride, sb, st, grad, xent_grad, w.y2d, S, T, P, pen_c2, row_w, device,
                      stream_v);
  if (rc != TC_OK || (!ragged && !o.isolate)) return rc;
  // A ragged minibatch: the objective wrote no padding row, the last passes moved whatever lay there; +0 into the padding
  // of the caller's gradients, each where its layout puts element (sequence, frame, channel).  (The (B, C, T) xent gradient
  // was cleared on the way in and has entries only at the numerator's posteriors.)
  const bool bct = layout == TC_LAYOUT_BCT;
  const int eb = half ? 2 : 4;
  const int64_t zb = bct || cl ? (int64_t)T * P : (int64_t)P, zt = bct ? 1 : (cl ? (int64_t)P : (int64_t)S * P), zc = bct ? T : 1;
  if (o.isolate) {
    // The isolating step: a failed sequence is a sequence of no frames.  The finalize left every sequence's surviving frames
    // in the workspace (its own length, 0 when it failed; the handle's lengths when the whole minibatch took the failure
    // route), so the one launch covers padding and failed sequences -- whose rows hold whatever the kernels made of a
    // non-finite recursion, the (B, C, T) xent gradient's included.
    rc = launch_zero_failed(grad, eb, zb, zt, zc, S, T, P, alive, stream);
    if (rc == TC_OK && xent_grad && use_xent) rc = launch_zero_failed(xent_grad, eb, zb, zt, zc, S, T, P, alive, stream);
    return rc;
  }
  rc = launch_zero_padding(grad, eb, zb, zt, zc, S, T, P, frames_dev, stream);
  if (rc == TC_OK && xent_grad && use_xent && !bct) rc = launch_zero_padding(xent_grad, eb, zb, zt, zc, S, T, P, frames_dev, stream);
  return rc;
}

int tc_chain_step(tc_den_graph *g, tc_supervision *sup, const float *input, const float *xent_input, int three_d,
                  int64_t row_stride, float l2_regularize, float leaky, float xent_regularize, int kaldi_way,
                  float *grad, float *xent_grad, float *results_dev3, float *loss_dev1, double *xent_objf_dev,
                  void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return chain_step_layout(g, sup, input, xent_input, three_d ? TC_LAYOUT_BCT : TC_LAYOUT_ROWS, row_stride, 0, 0, l2_regularize,
                           leaky, xent_regularize, kaldi_way, grad, xent_grad, results_dev3, loss_dev1, xent_objf_dev, nullptr,
                           0.0f, TC_DTYPE_F32, workspace, workspace_bytes, device, stream_v);
}

int tc_chain_step_typed(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int three_d,
                        int64_t row_stride, float l2_regularize, float leaky, float xent_regularize, int kaldi_way,
                        void *grad_v, void *xent_grad_v, float *results_dev3, float *loss_dev1, double *xent_objf_dev,
                        int dtype, void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return chain_step_layout(g, sup, input_v, xent_input_v, three_d ? TC_LAYOUT_BCT : TC_LAYOUT_ROWS, row_stride, 0, 0,
                           l2_regularize, leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1,
                           xent_objf_dev, nullptr, 0.0f, dtype, workspace, workspace_bytes, device, stream_v);
}

int tc_chain_step_weighted(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v,
                           int three_d, int64_t row_stride, float l2_regularize, float leaky, float xent_regularize,
                           int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3, float *loss_dev1,
                           double *xent_objf_dev, const float *deriv_weights, int dtype, void *workspace,
                           int64_t workspace_bytes, int device, void *stream_v) {
  return chain_step_layout(g, sup, input_v, xent_input_v, three_d ? TC_LAYOUT_BCT : TC_LAYOUT_ROWS, row_stride, 0, 0,
                           l2_regularize, leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1,
                           xent_objf_dev, deriv_weights, 0.0f, dtype, workspace, workspace_bytes, device, stream_v);
}

int tc_chain_step_penalized(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v,
                            int three_d, int64_t row_stride, float l2_regularize, float leaky, float xent_regularize,
                            int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3, float *loss_dev1,
                            double *xent_objf_dev, const float *deriv_weights, float out_of_range_regularize, int dtype,
                            void *workspace, int64_t workspace_bytes, int device, void *stream_v) {
  return chain_step_layout(g, sup, input_v, xent_input_v, three_d ? TC_LAYOUT_BCT : TC_LAYOUT_ROWS, row_stride, 0, 0,
                           l2_regularize, leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1,
                           xent_objf_dev, deriv_weights, out_of_range_regularize, dtype, workspace, workspace_bytes, device,
                           stream_v);
}

int64_t tc_chain_step_strided_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T, int layout, int with_xent,
                                              int dtype) {
  if (layout != TC_LAYOUT_ROWS && layout != TC_LAYOUT_BCT && layout != TC_LAYOUT_CHANNEL_LAST) return TC_ERR_INVALID_ARGUMENT;
  return tc_chain_step_typed_workspace_bytes(g, S, T, layout != TC_LAYOUT_ROWS, with_xent, dtype);
}

int64_t tc_chain_step_log_softmax_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T, int layout, int with_xent,
                                                  int dtype) {
  if (layout != TC_LAYOUT_ROWS && layout != TC_LAYOUT_BCT && layout != TC_LAYOUT_CHANNEL_LAST) return TC_ERR_INVALID_ARGUMENT;
  if (!g || S <= 0 || T <= 0 || !known_dtype(dtype)) return TC_ERR_INVALID_ARGUMENT;
  return (int64_t)carve_step(nullptr, g, S, T, g->P, layout != TC_LAYOUT_ROWS, with_xent != 0, dtype, true).total;
}

int tc_chain_step_per_sequence(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int layout,
                               int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize, float leaky,
                               float xent_regularize, int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3,
                               float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                               float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                               void *stream_v, int isolate_failures, double *seq_results_dev) {
  return tc_chain_step_log_softmax(g, sup, input_v, xent_input_v, layout, row_stride, batch_stride, frame_stride, l2_regularize,
                                   leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1,
                                   xent_objf_dev, deriv_weights, out_of_range_regularize, dtype, workspace, workspace_bytes,
                                   device, stream_v, isolate_failures, seq_results_dev, 0);
}

int tc_chain_step_log_softmax(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int layout,
                              int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize, float leaky,
                              float xent_regularize, int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3,
                              float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                              float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                              void *stream_v, int isolate_failures, double *seq_results_dev, int xent_log_softmax) {
  if (layout == TC_LAYOUT_ROWS || layout == TC_LAYOUT_BCT)
    return chain_step_layout(g, sup, input_v, xent_input_v, layout, row_stride, 0, 0, l2_regularize, leaky, xent_regularize,
                             kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1, xent_objf_dev, deriv_weights,
                             out_of_range_regularize, dtype, workspace, workspace_bytes, device, stream_v, isolate_failures,
                             seq_results_dev, xent_log_softmax);
  if (layout != TC_LAYOUT_CHANNEL_LAST || !sup) return TC_ERR_INVALID_ARGUMENT;
  if (!channel_last_strides_ok(sup->S, sup->T, sup->P, batch_stride, frame_stride)) return TC_ERR_INVALID_ARGUMENT;
  // (element offsets are multiples of the element size: a base that is not breaks every access)
  const uintptr_t elem_mask = dtype == TC_DTYPE_F32 ? 3 : 1;
  if ((((uintptr_t)input_v | (uintptr_t)xent_input_v | (uintptr_t)grad_v | (uintptr_t)xent_grad_v) & elem_mask) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  return chain_step_layout(g, sup, input_v, xent_input_v, layout, 0, batch_stride, frame_stride, l2_regularize, leaky,
                           xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1, xent_objf_dev,
                           deriv_weights, out_of_range_regularize, dtype, workspace, workspace_bytes, device, stream_v,
                           isolate_failures, seq_results_dev, xent_log_softmax);
}

int tc_chain_step_strided(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int layout,
                          int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize, float leaky,
                          float xent_regularize, int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3,
                          float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                          float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                          void *stream_v) {
  return tc_chain_step_per_sequence(g, sup, input_v, xent_input_v, layout, row_stride, batch_stride, frame_stride, l2_regularize,
                                    leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v, results_dev3, loss_dev1,
                                    xent_objf_dev, deriv_weights, out_of_range_regularize, dtype, workspace, workspace_bytes,
                                    device, stream_v, 0, nullptr);
}

// ---- boosted LF-MMI (boost_kernels.hip) -----------------------------------------------------------------------------
// the two forms of a_t(j) as the entries take them: exactly one of (ref, accuracy); classes with the hard form only
static bool boost_args_ok(float boost, const int32_t *ref, const int32_t *cls, const float *accuracy, int64_t accuracy_stride,
                          int P) {
  if (boost != boost || std::isinf(boost)) return false;
  if ((ref != nullptr) == (accuracy != nullptr)) return false;
  if (cls && !ref) return false;
  if ((((uintptr_t)ref | (uintptr_t)cls | (uintptr_t)accuracy) & 3) != 0) return false;
  return !accuracy || accuracy_stride >= P;
}

int64_t tc_chain_step_boosted_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T, int layout, int with_xent,
                                              int dtype) {
  if (layout != TC_LAYOUT_ROWS && layout != TC_LAYOUT_BCT && layout != TC_LAYOUT_CHANNEL_LAST) return TC_ERR_INVALID_ARGUMENT;
  if (!g || S <= 0 || T <= 0 || !known_dtype(dtype)) return TC_ERR_INVALID_ARGUMENT;
  return (int64_t)carve_step(nullptr, g, S, T, g->P, layout != TC_LAYOUT_ROWS, with_xent != 0, dtype, true, layout != TC_LAYOUT_BCT)
      .total;
}

int tc_chain_step_boosted(tc_den_graph *g, tc_supervision *sup, const void *input_v, const void *xent_input_v, int layout,
                          int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize, float leaky,
                          float xent_regularize, int kaldi_way, void *grad_v, void *xent_grad_v, float *results_dev3,
                          float *loss_dev1, double *xent_objf_dev, const float *deriv_weights, float out_of_range_regularize,
                          int dtype, void *workspace, int64_t workspace_bytes, int device, void *stream_v, int isolate_failures,
                          double *seq_results_dev, int xent_log_softmax, float boost, const int32_t *ref_pdfs_dev,
                          const int32_t *pdf_class_dev, const float *accuracy, int64_t accuracy_row_stride) {
  if (!sup) return TC_ERR_INVALID_ARGUMENT;
  if (!boost_args_ok(boost, ref_pdfs_dev, pdf_class_dev, accuracy, accuracy_row_stride, sup->P)) return TC_ERR_INVALID_ARGUMENT;
  if (layout != TC_LAYOUT_ROWS && layout != TC_LAYOUT_BCT && layout != TC_LAYOUT_CHANNEL_LAST) return TC_ERR_INVALID_ARGUMENT;
  const bool cl = layout == TC_LAYOUT_CHANNEL_LAST;
  if (cl) {
    if (!channel_last_strides_ok(sup->S, sup->T, sup->P, batch_stride, frame_stride)) return TC_ERR_INVALID_ARGUMENT;
    const uintptr_t elem_mask = dtype == TC_DTYPE_F32 ? 3 : 1;
    if ((((uintptr_t)input_v | (uintptr_t)xent_input_v | (uintptr_t)grad_v | (uintptr_t)xent_grad_v) & elem_mask) != 0)
      return TC_ERR_INVALID_ARGUMENT;
  }
  BoostAcc a;
  a.ref = ref_pdfs_dev;
  a.cls = pdf_class_dev;
  a.acc = accuracy;
  a.acc_stride = accuracy_row_stride;
  a.b = boost;
  return chain_step_layout(g, sup, input_v, xent_input_v, layout, cl ? 0 : row_stride, cl ? batch_stride : 0,
                           cl ? frame_stride : 0, l2_regularize, leaky, xent_regularize, kaldi_way, grad_v, xent_grad_v,
                           results_dev3, loss_dev1, xent_objf_dev, deriv_weights, out_of_range_regularize, dtype, workspace,
                           workspace_bytes, device, stream_v, isolate_failures, seq_results_dev, xent_log_softmax, &a);
}

int tc_boost_rows(const void *input, int dtype, int layout, int32_t S, int32_t Cn, int32_t T, int64_t row_stride,
                  int64_t batch_stride, int64_t frame_stride, const int32_t *seq_frames_dev, float boost,
                  const int32_t *ref_pdfs_dev, const int32_t *pdf_class_dev, const float *accuracy, int64_t accuracy_row_stride,
                  float *out2d, int64_t out_stride, int device, void *stream_v) {
  if (!input || !out2d || !known_dtype(dtype) || S <= 0 || Cn <= 0 || T <= 0 || out_stride < Cn) return TC_ERR_INVALID_ARGUMENT;
  if (!boost_args_ok(boost, ref_pdfs_dev, pdf_class_dev, accuracy, accuracy_row_stride, Cn)) return TC_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)input) & (dtype == TC_DTYPE_F32 ? 3 : 1)) != 0 || (((uintptr_t)out2d | (uintptr_t)seq_frames_dev) & 3) != 0)
    return TC_ERR_INVALID_ARGUMENT;
  int64_t sb = batch_stride, st = frame_stride;
  if (layout == TC_LAYOUT_ROWS) {
    if (row_stride < Cn || row_stride > INT64_MAX / 4 / S) return TC_ERR_INVALID_ARGUMENT;
    sb = row_stride;
    st = (int64_t)S * row_stride;
  } else if (layout != TC_LAYOUT_BCT && layout != TC_LAYOUT_CHANNEL_LAST) {
    return TC_ERR_INVALID_ARGUMENT;
  }
  if (layout != TC_LAYOUT_BCT && !channel_last_strides_ok(S, T, Cn, sb, st)) return TC_ERR_INVALID_ARGUMENT;
  if (layout == TC_LAYOUT_BCT && !layout_grid_ok(S, T)) return TC_ERR_UNSUPPORTED;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  BoostAcc a;
  a.ref = ref_pdfs_dev;
  a.cls = pdf_class_dev;
  a.acc = accuracy;
  a.acc_stride = accuracy_row_stride;
  a.b = boost;
  a.seq_frames = seq_frames_dev;
  if (layout == TC_LAYOUT_BCT) return launch_boost_bct(dtype, input, out2d, out_stride, S, Cn, T, a, (hipStream_t)stream_v);
  return launch_boost_rows(dtype, input, sb, st, out2d, out_stride, S, T, Cn, a, (hipStream_t)stream_v);
}

int tc_rows_gather(const void *in, int dtype, int32_t B, int32_t Cn, int32_t T, int64_t batch_stride, int64_t frame_stride,
                   float *out2d, int64_t out_stride, int device, void *stream_v) {
  if (!in || !out2d || !known_dtype(dtype) || B <= 0 || Cn <= 0 || T <= 0 || out_stride < Cn) return TC_ERR_INVALID_ARGUMENT;
  if (!channel_last_strides_ok(B, T, Cn, batch_stride, frame_stride)) return TC_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  return launch_rows_gather(dtype, in, batch_stride, frame_stride, out2d, out_stride, B, T, Cn, (hipStream_t)stream_v);
}

int tc_rows_scatter(const float *in2d, int64_t in_stride, int dtype, int32_t B, int32_t Cn, int32_t T, float scale,
                    const float *row_weights, float out_of_range_regularize, const void *input, int64_t batch_stride,
                    int64_t frame_stride, void *out_btc, int device, void *stream_v) {
  if (!in2d || !out_btc || !known_dtype(dtype) || B <= 0 || Cn <= 0 || T <= 0 || in_stride < Cn) return TC_ERR_INVALID_ARGUMENT;
  if (!(out_of_range_regularize >= 0.0f) || std::isinf(2.0f * out_of_range_regularize)) return TC_ERR_INVALID_ARGUMENT;
  const float pen_c2 = 2.0f * out_of_range_regularize;
  if (pen_c2 > 0.0f && (!input || !channel_last_strides_ok(B, T, Cn, batch_stride, frame_stride))) return TC_ERR_INVALID_ARGUMENT;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  LastPass lp;
  lp.scale = scale;
  lp.row_w = row_weights;
  lp.pen_c2 = pen_c2;
  lp.y = input;
  lp.y_stride = batch_stride;
  lp.y_st = frame_stride;
  return launch_rows_scatter(dtype, in2d, in_stride, out_btc, (int64_t)T * Cn, Cn, B, T, Cn, lp, (hipStream_t)stream_v);
}

int tc_xent_objf(const float *xent_output, int64_t rows, int32_t cols, int64_t output_stride, const float *xent_deriv,
                 int64_t deriv_stride, double *objf_dev, void *workspace, int64_t workspace_bytes, int device,
                 void *stream_v) {
  if (!xent_output || !xent_deriv || !objf_dev || rows <= 0 || cols <= 0 || output_stride < cols || deriv_stride < cols)
    return TC_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < trace_workspace_bytes() || !aligned16(workspace)) return TC_ERR_WORKSPACE;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  return launch_trace_mat_mat(xent_output, output_stride, xent_deriv, deriv_stride, rows, cols, (double *)workspace,
                              objf_dev, (hipStream_t)stream_v);
}

int tc_to2d(const float *in_bct, int32_t B, int32_t Cn, int32_t T, float *out2d, int64_t out_stride, int device,
            void *stream_v) {
  if (!in_bct || !out2d || B <= 0 || Cn <= 0 || T <= 0 || out_stride < Cn) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_grid_ok(B, T)) return TC_ERR_UNSUPPORTED;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  return launch_to2d(TC_DTYPE_F32, in_bct, out2d, B, Cn, T, out_stride, (hipStream_t)stream_v);
}

int tc_from2d(const float *in2d, int64_t in_stride, int32_t B, int32_t Cn, int32_t T, float scale, float *out_bct,
              int device, void *stream_v) {
  if (!in2d || !out_bct || B <= 0 || Cn <= 0 || T <= 0 || in_stride < Cn) return TC_ERR_INVALID_ARGUMENT;
  if (!layout_grid_ok(B, T)) return TC_ERR_UNSUPPORTED;
  DeviceGuard guard(device);
  if (!guard.ok) return TC_ERR_HIP;
  LastPass lp;
  lp.scale = scale;
  return launch_from2d(TC_DTYPE_F32, in2d, in_stride, out_bct, B, Cn, T, lp, (hipStream_t)stream_v);
}

}  // extern "C"
