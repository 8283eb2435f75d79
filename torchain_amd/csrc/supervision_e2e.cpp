// Host side of the end-to-end supervision ([K] Supervision::e2e_fsts, chain-supervision.h): one acceptor per sequence,
// not unfolded in time, whose numerator is [K] GenericNumeratorComputation (chain-generic-numerator.cc).  Kaldi walks
// these FSTs on the CPU after copying the numerator's rows of nnet_output to the host; here the host only validates them
// and lays out the tables the kernel (num_e2e_kernels.hip) walks: in-arcs by destination (forward), out-arcs by source
// (backward), the distinct pdfs of each sequence and, per pdf, its out-arcs in a fixed order (a deterministic posterior
// sum).  The tables and the kernel's scratch share one slot of the per-device supervision pool (supervision.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "chain_internal.h"

using namespace tc;

namespace tc {

namespace {
// The kernels' scratch behind the uploaded tables of a slot, each part rounded up to 256 bytes: the log-alpha history,
// y / the posteriors and -- `large`: for handles that take num_e2e_large_kernels.hip -- one float per arc.
struct E2eScratch { size_t alpha, stage, occ; };
E2eScratch e2e_scratch(const E2eTables &tb, int T, bool large) {
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  return {up((size_t)(T + 1) * tb.total_states * 8), up((size_t)T * tb.total_pdfs * 4), large ? up(std::max<size_t>(tb.in_key.size(), 1) * 4) : 0};
}
// launch_num_e2e's choice, made when the handle reaches a device (the slot's size) and again at every launch
bool e2e_takes_large(const E2eTables &tb) {
  return e2e_beyond_resident(tb.max_states, tb.max_arcs, tb.max_pdfs) || debug_flag(kDbgForceNumE2eLarge);
}
}  // namespace

// The host half of an upload (tc_supervision_stage) for an end-to-end supervision.  Caller holds sup->mu and has checked
// that the device has no slot yet.
int stage_e2e_locked(tc_supervision *sup, int device) {
  const E2eTables &tb = sup->e2e_tab;
  const int T = sup->T;
  const E2eScratch sc = e2e_scratch(tb, T, e2e_takes_large(tb));
  struct Part { const void *src; size_t bytes; };
  const Part parts[] = {
      {tb.state_off.data(), tb.state_off.size() * 4}, {tb.arc_off.data(), tb.arc_off.size() * 4},
      {tb.pdf_off.data(), tb.pdf_off.size() * 4},     {tb.start.data(), tb.start.size() * 4},
      {tb.in_begin.data(), tb.in_begin.size() * 4},   {tb.out_begin.data(), tb.out_begin.size() * 4},
      {tb.pdf_begin.data(), tb.pdf_begin.size() * 4}, {tb.pdf_arc.data(), tb.pdf_arc.size() * 4},
      {tb.pdf_of.data(), tb.pdf_of.size() * 4},       {tb.in_key.data(), tb.in_key.size() * 4},
      {tb.out_key.data(), tb.out_key.size() * 4},     {tb.in_lw.data(), tb.in_lw.size() * 4},
      {tb.out_lw.data(), tb.out_lw.size() * 4},       {tb.final_lw.data(), tb.final_lw.size() * 4},
      {sup->frames.data(), sup->frames.size() * 4},  // ragged handles: the sequences' lengths travel with the tables
  };
  const int nparts = (int)(sizeof(parts) / sizeof(parts[0]));
  size_t total = 0;
  sup->blob_off.clear();
  for (int i = 0; i < nparts; ++i) {
    sup->blob_off.push_back(total);
    total += (parts[i].bytes + 255) & ~(size_t)255;
  }
  total += 256;
  const size_t upload = total;
  // the kernel's scratch, sized with the slot (so tc_chain_workspace_bytes does not depend on the supervision's kind)
  const size_t alpha_off = total;
  total += sc.alpha;
  const size_t stage_off = total;
  total += sc.stage;
  const size_t occ_off = total;  // (the large kernel's arc occupations: only in the slots of handles that take it)
  total += sc.occ;
  PoolSlot *slot = nullptr;
  int rc = pool_acquire(device, total, &slot);
  if (rc != TC_OK) return rc;
  for (int i = 0; i < nparts; ++i)
    if (parts[i].bytes) memcpy(slot->host + sup->blob_off[i], parts[i].src, parts[i].bytes);
  NumDev d;
  d.slot = slot;
  d.upload_bytes = upload;
  d.uploaded = false;
  d.e2e = 1;
  char *blob = slot->blob;
  auto P = [&](int i) { return (const int32_t *)(blob + sup->blob_off[i]); };
  E2eDev &e = d.e2e_tab;
  e.state_off = P(0); e.arc_off = P(1); e.pdf_off = P(2); e.start = P(3); e.in_begin = P(4); e.out_begin = P(5);
  e.pdf_begin = P(6); e.pdf_arc = P(7); e.pdf_of = P(8);
  e.in_key = (const uint32_t *)P(9);
  e.out_key = (const uint32_t *)P(10);
  e.in_lw = (const float *)P(11);
  e.out_lw = (const float *)P(12);
  e.final_lw = (const float *)P(13);
  e.alpha_hist = (double *)(blob + alpha_off);
  e.max_states = tb.max_states;
  e.max_arcs = tb.max_arcs;
  e.max_pdfs = tb.max_pdfs;
  e.occ_off256 = sc.occ ? (int32_t)((occ_off - alpha_off) / 256) : 0;  // (both multiples of 256; the scratch is below 4 GiB + 4 * arcs)
  d.stage = (float *)(blob + stage_off);
  sup->dev[device] = d;
  if (!sup->frames.empty()) sup->frames_dev[device] = P(14);
  return TC_OK;
}

}  // namespace tc

namespace {

// T: frames of every sequence, or -- seq_frames given (S entries, each 1..T) -- of the longest: the T of every shape, row
// count, workspace and scratch rule.  A handle made with seq_frames is ragged whatever the lengths are.
// any_size (tc_supervision_create_e2e_any): the size rule is the large kernel's LDS, not the resident kernel's limits.
int create_e2e(tc_supervision **out, float weight, int32_t S, int32_t T, const int32_t *seq_frames, int32_t label_dim, bool any_size,
               const int32_t *seq_state_begin, const int32_t *start, const int32_t *arc_begin, const int32_t *ilabel,
               const float *arc_weight, const int32_t *nextstate, const float *final_weight) {
  if (S <= 0 || T <= 0 || label_dim <= 0 || !seq_state_begin || !start || !arc_begin || !final_weight)
    return TC_ERR_INVALID_ARGUMENT;
  if ((int64_t)S * T > ((int64_t)1 << 26)) return TC_ERR_UNSUPPORTED;  // the egs readers' bound on a minibatch
  if (seq_state_begin[0] != 0) return TC_ERR_BAD_FST;
  for (int32_t s = 0; s < S; ++s)
    if (seq_state_begin[s + 1] < seq_state_begin[s]) return TC_ERR_BAD_FST;
  const int32_t num_states = seq_state_begin[S];
  if (arc_begin[0] != 0) return TC_ERR_BAD_FST;
  for (int32_t g = 0; g < num_states; ++g)
    if (arc_begin[g + 1] < arc_begin[g]) return TC_ERR_BAD_FST;
  const int32_t num_arcs = arc_begin[num_states];
  if (num_arcs > 0 && (!ilabel || !arc_weight || !nextstate)) return TC_ERR_INVALID_ARGUMENT;

  // structure first (TC_ERR_BAD_FST), then the kernel's size limits (TC_ERR_UNSUPPORTED)
  bool too_large = false;
  std::vector<int32_t> upid_of(label_dim, -1), touched;
  for (int32_t s = 0; s < S; ++s) {
    const int32_t sb = seq_state_begin[s], n = seq_state_begin[s + 1] - sb;
    if (start[s] < 0 || start[s] >= n) return TC_ERR_BAD_FST;
    bool any_final = false;
    for (int32_t i = 0; i < n; ++i) {
      const float f = final_weight[sb + i];
      if (std::isnan(f) || f == -std::numeric_limits<float>::infinity()) return TC_ERR_BAD_FST;
      if (!std::isinf(f)) any_final = true;
    }
    if (!any_final) return TC_ERR_BAD_FST;
    int32_t npdf = 0;
    for (int32_t a = arc_begin[sb]; a < arc_begin[sb + n]; ++a) {
      if (ilabel[a] < 1 || ilabel[a] > label_dim) return TC_ERR_BAD_FST;  // 0: epsilon
      if (nextstate[a] < 0 || nextstate[a] >= n) return TC_ERR_BAD_FST;
      if (std::isnan(arc_weight[a]) || arc_weight[a] == -std::numeric_limits<float>::infinity()) return TC_ERR_BAD_FST;
      if (upid_of[ilabel[a] - 1] < 0) {
        upid_of[ilabel[a] - 1] = npdf++;
        touched.push_back(ilabel[a] - 1);
      }
    }
    for (int32_t p : touched) upid_of[p] = -1;
    touched.clear();
    if (any_size ? !e2e_large_fits(n, npdf) : e2e_beyond_resident(n, arc_begin[sb + n] - arc_begin[sb], npdf)) too_large = true;
  }
  if (too_large) return TC_ERR_UNSUPPORTED;
  // the kernel's scratch in the supervision's pool slot (stage_e2e_locked): the log-alpha history, (T + 1) x states
  // doubles, and y / the posteriors, T x distinct pdfs floats -- bounded here, not at the first step's allocation
  {
    int64_t pdfs = 0;
    for (int32_t s = 0; s < S; ++s) {
      for (int32_t a = arc_begin[seq_state_begin[s]]; a < arc_begin[seq_state_begin[s + 1]]; ++a)
        if (upid_of[ilabel[a] - 1] < 0) upid_of[ilabel[a] - 1] = 0, touched.push_back(ilabel[a] - 1), ++pdfs;
      for (int32_t p : touched) upid_of[p] = -1;
      touched.clear();
    }
    if ((double)(T + 1) * num_states * 8 + (double)T * pdfs * 4 > (double)kE2eMaxScratchBytes) return TC_ERR_UNSUPPORTED;
  }

  tc_supervision *sup = new tc_supervision();
  sup->e2e = true;
  sup->weight = weight;
  sup->S = S;
  sup->T = T;
  sup->P = label_dim;
  sup->total_frames = (int64_t)S * T;
  if (seq_frames) {
    sup->frames.assign(seq_frames, seq_frames + S);
    sup->total_frames = 0;
    for (int32_t s = 0; s < S; ++s) sup->total_frames += seq_frames[s];
  }
  E2eTables &tb = sup->e2e_tab;
  tb.state_off.assign(seq_state_begin, seq_state_begin + S + 1);
  tb.start.assign(start, start + S);
  tb.arc_off.push_back(0);
  tb.pdf_off.push_back(0);
  tb.in_key.reserve(num_arcs);
  tb.in_lw.reserve(num_arcs);
  tb.out_key.reserve(num_arcs);
  tb.out_lw.reserve(num_arcs);
  tb.pdf_arc.reserve(num_arcs);
  tb.final_lw.reserve(num_states);
  std::vector<int32_t> cnt, fill, arc_upid;
  for (int32_t s = 0; s < S; ++s) {
    const int32_t sb = seq_state_begin[s], n = seq_state_begin[s + 1] - sb;
    const int32_t a0 = arc_begin[sb], na = arc_begin[sb + n] - a0;
    for (int32_t i = 0; i < n; ++i) {
      const float f = final_weight[sb + i];
      tb.final_lw.push_back(-f);  // (+inf: not final -> -inf)
    }
    // distinct pdfs in first-occurrence order over the out-arcs
    const int32_t ubase = (int32_t)tb.pdf_of.size();
    arc_upid.resize(na);
    for (int32_t k = 0; k < na; ++k) {
      const int32_t pdf = ilabel[a0 + k] - 1;
      if (upid_of[pdf] < 0) {
        upid_of[pdf] = (int32_t)tb.pdf_of.size() - ubase;
        tb.pdf_of.push_back(pdf);
      }
      arc_upid[k] = upid_of[pdf];
    }
    const int32_t npdf = (int32_t)tb.pdf_of.size() - ubase;
    for (int32_t u = 0; u < npdf; ++u) upid_of[tb.pdf_of[ubase + u]] = -1;
    // out-arcs: the input's order (by source)
    for (int32_t i = 0; i <= n; ++i) tb.out_begin.push_back(arc_begin[sb + i] - a0);
    for (int32_t k = 0; k < na; ++k) {
      tb.out_key.push_back((uint32_t)nextstate[a0 + k] | ((uint32_t)arc_upid[k] << 16));
      tb.out_lw.push_back(-arc_weight[a0 + k]);
    }
    // in-arcs by destination, stable by arc position
    cnt.assign(n + 1, 0);
    for (int32_t k = 0; k < na; ++k) cnt[nextstate[a0 + k] + 1]++;
    for (int32_t i = 0; i < n; ++i) cnt[i + 1] += cnt[i];
    for (int32_t i = 0; i <= n; ++i) tb.in_begin.push_back(cnt[i]);
    fill.assign(cnt.begin(), cnt.end() - 1);
    std::vector<int32_t> order(na);
    for (int32_t k = 0; k < na; ++k) order[fill[nextstate[a0 + k]]++] = k;
    std::vector<int32_t> src_of(na);
    for (int32_t i = 0; i < n; ++i)
      for (int32_t k = arc_begin[sb + i] - a0; k < arc_begin[sb + i + 1] - a0; ++k) src_of[k] = i;
    for (int32_t j = 0; j < na; ++j) {
      const int32_t k = order[j];
      tb.in_key.push_back((uint32_t)src_of[k] | ((uint32_t)arc_upid[k] << 16));
      tb.in_lw.push_back(tb.out_lw[tb.out_lw.size() - na + k]);
    }
    // per pdf: its out-arc positions, increasing
    cnt.assign(npdf + 1, 0);
    for (int32_t k = 0; k < na; ++k) cnt[arc_upid[k] + 1]++;
    for (int32_t u = 0; u < npdf; ++u) cnt[u + 1] += cnt[u];
    for (int32_t u = 0; u <= npdf; ++u) tb.pdf_begin.push_back(cnt[u]);
    const size_t pb = tb.pdf_arc.size();
    tb.pdf_arc.resize(pb + na);
    for (int32_t k = 0; k < na; ++k) tb.pdf_arc[pb + cnt[arc_upid[k]]++] = k;
    tb.arc_off.push_back(tb.arc_off.back() + na);
    tb.pdf_off.push_back(tb.pdf_off.back() + npdf);
    tb.max_states = std::max(tb.max_states, n);
    tb.max_arcs = std::max(tb.max_arcs, na);
    tb.max_pdfs = std::max(tb.max_pdfs, npdf);
  }
  tb.total_states = num_states;
  tb.total_pdfs = tb.pdf_off.back();
  *out = sup;
  return TC_OK;
}

}  // namespace

extern "C" {

int tc_supervision_create_e2e(tc_supervision **out, float weight, int32_t S, int32_t T, int32_t label_dim,
                              const int32_t *seq_state_begin, const int32_t *start, const int32_t *arc_begin,
                              const int32_t *ilabel, const float *arc_weight, const int32_t *nextstate,
                              const float *final_weight) {
  if (!out) return TC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return create_e2e(out, weight, S, T, nullptr, label_dim, false, seq_state_begin, start, arc_begin, ilabel, arc_weight, nextstate,
                    final_weight);
}

int tc_supervision_create_e2e_ragged(tc_supervision **out, float weight, int32_t S, const int32_t *frames_per_sequence,
                                     int32_t label_dim, const int32_t *seq_state_begin, const int32_t *start,
                                     const int32_t *arc_begin, const int32_t *ilabel, const float *arc_weight,
                                     const int32_t *nextstate, const float *final_weight) {
  if (!out) return TC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (S <= 0 || !frames_per_sequence) return TC_ERR_INVALID_ARGUMENT;
  int32_t tmax = 0;
  for (int32_t s = 0; s < S; ++s) {
    if (frames_per_sequence[s] < 1) return TC_ERR_INVALID_ARGUMENT;
    tmax = std::max(tmax, frames_per_sequence[s]);
  }
  return create_e2e(out, weight, S, tmax, frames_per_sequence, label_dim, false, seq_state_begin, start, arc_begin, ilabel,
                    arc_weight, nextstate, final_weight);
}

int tc_supervision_create_e2e_any(tc_supervision **out, float weight, int32_t S, int32_t frames_per_sequence,
                                  const int32_t *seq_frames, int32_t label_dim, const int32_t *seq_state_begin,
                                  const int32_t *start, const int32_t *arc_begin, const int32_t *ilabel,
                                  const float *arc_weight, const int32_t *nextstate, const float *final_weight) {
  if (!out) return TC_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int32_t T = frames_per_sequence;
  if (seq_frames) {
    if (S <= 0) return TC_ERR_INVALID_ARGUMENT;
    T = 0;
    for (int32_t s = 0; s < S; ++s) {
      if (seq_frames[s] < 1) return TC_ERR_INVALID_ARGUMENT;
      T = std::max(T, seq_frames[s]);
    }
  }
  return create_e2e(out, weight, S, T, seq_frames, label_dim, true, seq_state_begin, start, arc_begin, ilabel, arc_weight,
                    nextstate, final_weight);
}

int tc_supervision_e2e_stats(const tc_supervision *s, int64_t *out) {
  if (!s || !out || !s->e2e) return TC_ERR_INVALID_ARGUMENT;
  const E2eTables &tb = s->e2e_tab;
  const bool large = e2e_takes_large(tb);
  const E2eScratch sc = e2e_scratch(tb, s->T, large);
  out[0] = s->S;
  out[1] = tb.max_states;
  out[2] = tb.max_arcs;
  out[3] = tb.max_pdfs;
  out[4] = (int64_t)num_e2e_lds_bytes(tb.max_states, tb.max_arcs, tb.max_pdfs);
  // (the large kernel and the best path lay their LDS out per sequence: the most one sequence needs)
  size_t seq_lds = 0;
  for (int32_t q = 0; q < s->S; ++q)
    seq_lds = std::max(seq_lds, num_e2e_lds_bytes(tb.state_off[q + 1] - tb.state_off[q], 0, tb.pdf_off[q + 1] - tb.pdf_off[q]));
  out[5] = (int64_t)seq_lds;
  out[6] = (int64_t)(sc.alpha + sc.stage + sc.occ);
  out[7] = large ? 1 : 0;
  return TC_OK;
}

int tc_supervision_frames(const tc_supervision *s, int32_t *out_host) {
  if (!s || !out_host) return TC_ERR_INVALID_ARGUMENT;
  for (int32_t i = 0; i < s->S; ++i) out_host[i] = s->frames.empty() ? s->T : s->frames[i];
  return TC_OK;
}

int32_t tc_supervision_is_ragged(const tc_supervision *s) { return s && !s->frames.empty() ? 1 : 0; }

int32_t tc_supervision_is_e2e(const tc_supervision *s) { return s && s->e2e ? 1 : 0; }

}  // extern "C"
